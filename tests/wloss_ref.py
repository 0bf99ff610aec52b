"""Oracle of the per-pixel weighted training losses (resdepth_amd.masked_loss(..., weight=w)) and of the weight tiles of a
training batch, written from their definition (include/resdepth_hip_wloss.h), on the host.

The residual r comes from tests/loss_ref.py (fp32 with the kernels' roundings, so every sign and branch is the kernels');
everything after r is float64.  Nothing here is derived from the kernels: the pair terms are written with shifted slices, the
weights enter as omega = (w_a + w_b) / 2 per pair and w per pixel."""
import numpy as np
import torch

import loss_ref


def pair_terms_w(r, m, w64):
    """S = sum omega |r_a - r_b| (float64), Q = sum omega, K [N,1,H,W] = sum omega sign(r_e - r_other) over the valid pairs that
    contain e.  r fp32 (differences are ONE fp32 subtraction), m bool, w64 float64."""
    K = torch.zeros(r.shape, dtype=torch.float64)
    S = Q = 0.0
    for dim in (3, 2):                                       # horizontal pairs, then vertical pairs
        n = r.shape[dim]
        a, b = slice(0, n - 1), slice(1, n)
        ia = (Ellipsis, a) if dim == 3 else (Ellipsis, a, slice(None))
        ib = (Ellipsis, b) if dim == 3 else (Ellipsis, b, slice(None))
        d = r[ia] - r[ib]                                    # fp32
        v = (m[ia] & m[ib]).double()
        om = 0.5 * (w64[ia] + w64[ib]) * v
        S += float((om * d.double().abs()).sum())
        Q += float(om.sum())
        s = torch.sign(d).double() * om
        K[ia] += s
        K[ib] -= s
    return S, Q, K


def weighted_loss_oracle(y_pred, y, mask, weight, mean, std, kind="l1", delta=1.0, slope_weight=0.0, gout=1.0):
    """-> dict(loss, mae: python floats; g_data, g_slope: float64 [N,1,H,W], the two parts of d loss / d y_pred times gout;
    A, C, D, S, Q, Wc, K, r, m)."""
    r = loss_ref.residual(y_pred, y, mean, std)
    assert r.dim() == 4 and r.shape[1] == 1
    n = r.shape[0]
    m = mask.detach().cpu().reshape(r.shape) != 0
    w64 = weight.detach().cpu().to(torch.float32).reshape(r.shape).double()
    m64, r64 = m.double(), r.double()
    sd = std.detach().cpu().to(torch.float32).double().reshape(n, 1, 1, 1)
    rho, drho = loss_ref.rho_and_slope(r64, kind, float(delta))
    A, C = float((m64 * r64.abs()).sum()), float(m64.sum())
    D, Wc = float((m64 * w64 * rho).sum()), float((m64 * w64).sum())
    S, Q, K = pair_terms_w(r, m, w64)
    lam = float(slope_weight)
    with_slope = lam > 0.0 and Q > 0.0
    nan = float("nan")
    loss = (D / Wc if Wc > 0.0 else nan) + (lam * S / Q if with_slope else 0.0)
    g_data = gout * sd * m64 * w64 * drho / Wc if Wc > 0.0 else torch.zeros_like(r64)
    g_slope = gout * sd * (lam / Q) * K if with_slope else torch.zeros_like(r64)
    return dict(loss=loss, mae=A / C if C > 0.0 else nan, g_data=g_data, g_slope=g_slope, A=A, C=C, D=D, S=S, Q=Q, Wc=Wc, K=K,
                r=r, m=m)


def weight_tile(raster, table, pos, tile, aug):
    """The weight tile of one sample on the host: numpy crop of `raster` ([H, W] float32 weights, or uint8 classes with `table`)
    at pos = (y, x), the table lookup, then oracle.sample_oracle.augment with aug = (k, flip_v, flip_h) -> [tile, tile] float32."""
    from oracle.sample_oracle import augment
    y, x = int(pos[0]), int(pos[1])
    crop = np.asarray(raster)[y:y + tile, x:x + tile]
    assert crop.shape == (tile, tile)
    if table is not None:
        crop = np.asarray(table, dtype=np.float32)[crop.astype(np.int64)]
    k, fv, fh = aug
    return augment(crop.astype(np.float32)[None], int(k), bool(fv), bool(fh))[0]
