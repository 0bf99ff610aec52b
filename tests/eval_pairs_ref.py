"""numpy restatement of the evaluation of all pair planes of a sweep (TEST INFRASTRUCTURE ONLY): tests/eval_classes_ref.py
`classify` per plane, then `stats_row` per plane and on the concatenation of the planes' residuals and validity -- the pool of
test.py:288-313.  Pinned by tests/golden/g22_pairs_eval.npz (the reference's own evaluate_performance / get_statistics)."""
import numpy as np

import eval_classes_ref as R


def stats_row(r, valid, thr=None):
    """R.stats_row, with the record the library promises for an empty set (count 0, NaN elsewhere) where the restatement
    underneath has none: numpy's max / min of nothing raise."""
    r, valid = np.asarray(r).ravel(), np.asarray(valid).ravel()
    if not valid.any():
        return [0.0] + [np.nan] * 7 + ([0.0] + [np.nan] * 5 if thr else [np.nan] * 6)
    if thr and not (valid & (np.abs(r) <= thr)).any():
        return R.stats_row(r, valid)[:8] + [0.0] + [np.nan] * 5
    return R.stats_row(r, valid, thr)


def restate(pairs, init, gt, nodata, area=None, gt_mask=None, building=None, water=None, forest=None, thr=None, fused=None):
    """-> {'classes': names, 'before': [C, 14], 'pairs': [P, C, 14], 'pooled': [C, 14][, 'fused': [C, 14]]}"""
    kw = dict(init=init, gt=gt, nodata=nodata, area=area, gt_mask=gt_mask, building=building, water=water, forest=forest)
    per = [R.classify(pred=p, **kw) for p in pairs]
    names = [c for c in R.CLASSES if c in per[0][2]]
    out = {"classes": names,
           "before": np.array([stats_row(per[0][0], per[0][2][c][0], thr) for c in names]),
           "pairs": np.array([[stats_row(ra, cl[c][1], thr) for c in names] for _, ra, cl in per]),
           "pooled": np.array([stats_row(np.concatenate([ra.ravel() for _, ra, _ in per]),
                                           np.concatenate([cl[c][1].ravel() for _, _, cl in per]), thr) for c in names])}
    if fused is not None:
        _, rf, cf = R.classify(pred=fused, **kw)
        out["fused"] = np.array([stats_row(rf, cf[c][1], thr) for c in names])
    return out


def rows_of(by_class, classes, thr):
    """{class: stats} of evaluate_pairs_statistics -> [C, 14] in the column order of R.stats_row"""
    out = []
    for c in classes:
        st = by_class[c]
        row = [st[k] for k in R.KEYS]
        row += [st["truncated"][k] for k in R.TKEYS] if thr else [np.nan] * len(R.TKEYS)
        out.append(row)
    return np.array(out)


def g22_case(g):
    """the inputs of g22_pairs_eval.npz as restatement arguments (masks rebuilt as the uint8 rasters 0 / 1 / 255 the
    reference was given, each with the nodata value 255) -> (kwargs of restate, area rows)"""
    shape = g["gt"].shape
    n = g["gt"].size

    def mask(k):
        on = np.unpackbits(g[f"mask_{k}/set"])[:n].reshape(shape)
        nd = np.unpackbits(g[f"mask_{k}/nodata"])[:n].reshape(shape)
        return np.where(nd != 0, 255, on).astype(np.uint8), 255.0
    return dict(pairs=g["pairs"], init=g["init"], gt=g["gt"], nodata=float(g["nodata"]), area=g["area"], gt_mask=mask("g"),
                building=mask("b"), water=mask("w"), forest=mask("f"), thr=float(g["thr"]))


def area_defn(area):
    return None if area is None else {"x_extent": [(int(a[0]), int(a[1])) for a in area],
                                      "y_extent": [(int(a[2]), int(a[3])) for a in area]}
