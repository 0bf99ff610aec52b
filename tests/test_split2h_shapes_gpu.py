"""The three-product GEMM bodies (split2h) at every kernel's edge shapes (-m gpu).

tests/test_ops_gpu.py walks the kernel-selection rules with untagged operands (six products); tests/test_split2h_gpu.py checks the
three-product arithmetic on a few full-tile shapes.  This file joins the two: a case LEDGER of (op family, shape, knob overrides,
expected kernel class), every operand built with ops.amax_of / ops.pack_* so that both magnitude slots exist.  Per row:

  * the kernel under test ran: the class string the launch site hands the profiler (rd_prof_*) equals the ledger's;
  * the three-product body ran: out3 differs from the six-product result in some last bit -- rows marked three=False are the
    launches that have no split kernel at all (exact-f32 kernels: transposed convolutions of K <= 128 on the generic row tiles,
    weight-gradient TN tiles other than 128 x 128; include/resdepth_hip.h, rd_quant_next), there out3 == out6 bit for bit;
  * per OUTPUT ELEMENT, N(0,1) operands (gradients N(0,1) * 1e-5): |out3 - ref64| <= 16 u den + 2.5 |exact - ref64|, u = 2^-24,
    den = the op on |a|, |b| in fp64, exact = the exact-f32 kernels' result: the bar of tests/test_split2h_gpu.py (12 u analytic +
    4 u slack + what the fp32 accumulation of this K does anyway), held by every border row, ragged tile and channel tail;
  * one all-positive row per kernel class (a hi / lo accumulator mix-up shows there) on that file's tensor-level bars;
  * a second run gives the same bits; producers (conv data gradient, transposed-convolution forward) leave exactly max |out| in
    their slot -- ragged tiles are where a dead lane could leak into it.

The fused entry points follow (statistics epilogues, BN-backward hooks, BN + skip, folded inference with per-tensor and per-image
slots, staged epilogues), all in mode 3 with slots, against fp64 computed from the inputs (and from the kernel's own z where the
statistic is one OF z).  Every knob is restored by the `lib` fixture."""
import collections
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24

KNOBS = ("mfma_products", "mfma_f32", "nt_tile", "nt_halo", "nt_splitk", "nt_epi", "tn_tile", "tn_split", "wg_strip", "wg_occ",
         "convt_patch")


@pytest.fixture()
def lib():
    from resdepth_amd import _lib
    _lib.load()
    before = {k: _lib.tune_get(k) for k in KNOBS}
    prof = _lib.prof_level_py()
    _lib.tune_set("mfma_products", 3)
    _lib.tune_set("mfma_f32", 0)
    _lib.ensure_splitk_workspace(DEV)
    yield _lib
    for k, v in before.items():
        _lib.tune_set(k, v)
    _lib.prof_enable(prof)


class _knobs:
    """knob overrides for the duration of a block (the fixture restores the rest)"""

    def __init__(self, lib, kv):
        self.lib, self.kv = lib, dict(kv)

    def __enter__(self):
        self.old = {k: self.lib.tune_get(k) for k in self.kv}
        for k, v in self.kv.items():
            self.lib.tune_set(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.lib.tune_set(k, v)


def _slot_max(t):
    """largest of the sixteen words of a tensor's magnitude slot, as a float"""
    s = t._rd_amax.view(16, 32)[:, 0].max().item()
    return torch.tensor([s], dtype=torch.int32).view(torch.float32).item()


# ---- the ledger ------------------------------------------------------------------------------------------------------------
Row = collections.namedtuple("Row", "fam shape knobs cls three flavour")


def R(fam, shape, cls, three=True, **knobs):
    return Row(fam, shape, tuple(sorted(knobs.items())), cls, three, "randn")


def _nt(op, tile, amode, epi):
    return "%s|igemm_nt_split<%s,%d,%d>" % (op, tile, amode, epi)


T0, T1, T2 = "128,128", "128,64", "64,64"
FW, DG, WG = "conv3x3_fwd", "conv3x3_dgrad", "conv3x3_wgrad"
TFW, TDG, TWG = "convt2x2_fwd", "convt2x2_dgrad", "convt2x2_wgrad"
STRIP = WG + "|wgrad_strip_tr<%s>"

LEDGER = [
    # conv3_halo_split<64>: ragged Cout, 16-channel chunk tail (forward: Cin = 20; data gradient: Cout = 36 -> chunks 16 + 16 + 4)
    R("conv_fwd", (16, 64, 64, 20, 36), FW + "|conv3_halo_split<64>"),
    R("conv_dgrad", (16, 64, 64, 20, 36), DG + "|conv3_halo_split<64>"),
    # conv3_halo_split<128>: ragged N tile (132 of 256 columns); 5 x 6 patches per image; the same kernel as a data gradient
    R("conv_fwd", (16, 64, 64, 24, 132), FW + "|conv3_halo_split<128>"),
    R("conv_dgrad", (16, 64, 64, 24, 132), DG + "|conv3_halo_split<64>"),
    R("conv_dgrad", (16, 64, 64, 132, 24), DG + "|conv3_halo_split<128>"),
    R("conv_fwd", (16, 40, 96, 24, 132), FW + "|conv3_halo_split<128>"),
    # 48 x 80 images: 6 x 5 patches; at this batch the planner takes row tiles, nt_tile puts the shape on either patch kernel
    R("conv_fwd", (2, 48, 80, 64, 128), _nt(FW, T2, 0, 0)),
    R("conv_fwd", (2, 48, 80, 64, 128), FW + "|conv3_halo_split<128>", nt_tile=0),
    R("conv_fwd", (2, 48, 80, 64, 128), FW + "|conv3_halo_split<64>", nt_tile=1),
    R("conv_dgrad", (2, 48, 80, 64, 128), DG + "|conv3_halo_split<64>", nt_tile=1),
    R("conv_dgrad", (2, 48, 80, 128, 64), DG + "|conv3_halo_split<128>", nt_tile=0),
    R("conv_fwd", (2, 8, 16, 8, 24), FW + "|conv3_halo_split<64>", nt_tile=1),         # one patch per image, half a K chunk
    # 8 x 8 images: two images per patch, K in ranges of 8 chunks (split over blocks: rd_set_splitk_workspace); nt_splitk = 0
    # sends the layer to the row tiles; fewer than 8 chunks (Cin = 64) never reach the form
    R("conv_fwd", (32, 8, 8, 512, 512), FW + "|conv3_halo_split<64,w8>"),
    R("conv_dgrad", (32, 8, 8, 512, 512), DG + "|conv3_halo_split<64,w8>"),
    R("conv_fwd", (32, 8, 8, 512, 512), _nt(FW, T2, 0, 0), nt_splitk=0),
    R("conv_fwd", (33, 8, 8, 256, 64), FW + "|conv3_halo_split<64,w8>"),               # odd image count: the last pair is half empty
    R("conv_dgrad", (33, 8, 8, 64, 256), DG + "|conv3_halo_split<64,w8>"),
    R("conv_dgrad", (33, 8, 8, 64, 256), _nt(DG, T2, 0, 0), nt_splitk=0),
    R("conv_fwd", (33, 8, 8, 64, 256), _nt(FW, T2, 0, 0)),
    R("conv_fwd", (1, 8, 8, 64, 64), _nt(FW, T2, 0, 0)),
    R("conv_dgrad", (1, 8, 8, 64, 64), _nt(DG, T2, 0, 0)),
    # igemm_nt_split at every tile on shapes the patch kernels refuse (W % 16 != 0 or H % 8 != 0)
    R("conv_fwd", (1, 6, 48, 32, 128), _nt(FW, T0, 0, 0), nt_tile=0),
    R("conv_fwd", (1, 6, 48, 32, 128), _nt(FW, T1, 0, 0), nt_tile=1),
    R("conv_fwd", (1, 6, 48, 32, 128), _nt(FW, T2, 0, 0)),
    R("conv_dgrad", (1, 6, 48, 128, 32), _nt(DG, T0, 0, 0), nt_tile=0),
    R("conv_fwd", (2, 24, 40, 32, 64), _nt(FW, T1, 0, 0), nt_tile=1),
    R("conv_fwd", (2, 24, 40, 32, 64), _nt(FW, T2, 0, 0)),
    R("conv_dgrad", (2, 24, 40, 32, 64), _nt(DG, T1, 0, 0), nt_tile=1),
    R("conv_dgrad", (2, 24, 40, 32, 64), _nt(DG, T2, 0, 0)),
    R("conv_fwd", (3, 12, 20, 8, 24), _nt(FW, T1, 0, 0), nt_tile=1),
    R("conv_fwd", (3, 12, 20, 8, 24), _nt(FW, T2, 0, 0)),
    R("conv_dgrad", (3, 12, 20, 8, 24), _nt(DG, T1, 0, 0), nt_tile=1),
    R("conv_dgrad", (3, 12, 20, 8, 24), _nt(DG, T2, 0, 0)),
    R("conv_fwd", (2, 8, 16, 8, 24), _nt(FW, T2, 0, 0)),
    R("conv_dgrad", (2, 8, 16, 8, 24), _nt(DG, T2, 0, 0)),
    R("conv_fwd", (1, 4, 4, 4, 4), _nt(FW, T2, 0, 0)),
    R("conv_dgrad", (1, 4, 4, 4, 4), _nt(DG, T2, 0, 0)),
    # wgrad_strip_tr<2,2,2>: the rotating three-product body
    R("conv_wgrad", (1, 8, 16, 64, 128), STRIP % "2,2,2"),                             # the smallest image it takes
    R("conv_wgrad", (1, 256, 16, 64, 128), STRIP % "2,2,2"),                           # row chunks
    R("conv_wgrad", (2, 16, 32, 192, 320), STRIP % "2,2,2"),                           # 5 x 3 tiles
    R("conv_wgrad", (4, 16, 16, 128, 128), STRIP % "2,2,2"),                           # several strips per block
    R("conv_wgrad", (4, 16, 16, 128, 128), STRIP % "1,2,2", wg_occ=1),
    R("conv_wgrad", (1, 6, 48, 64, 128), STRIP % "2,2,2"),                             # 6 rows
    # <2,4,1>: un-swapped with a masked channel block, swapped roles (Cout < 128 <= Cin)
    R("conv_wgrad", (2, 32, 32, 32, 132), STRIP % "2,4,1"),
    R("conv_wgrad", (2, 32, 32, 32, 132), STRIP % "1,4,1", wg_occ=1),
    R("conv_wgrad", (4, 32, 32, 96, 160), STRIP % "2,4,1"),
    R("conv_wgrad", (2, 16, 32, 160, 32), STRIP % "2,4,1"),
    R("conv_wgrad", (4, 32, 32, 160, 32), STRIP % "2,4,1"),
    # <2,2,2,w8>: image pairs as strips
    R("conv_wgrad", (33, 8, 8, 64, 256), STRIP % "2,2,2,w8"),
    R("conv_wgrad", (1, 8, 8, 64, 64), STRIP % "2,2,2,w8"),
    R("conv_wgrad", (1, 8, 8, 64, 64), STRIP % "1,2,2,w8", wg_occ=1),
    R("conv_wgrad", (5, 8, 8, 128, 192), STRIP % "2,2,2,w8"),
    # TN kernels on shapes the strip kernel refuses: only 128 x 128 tiles are split kernels by themselves (tn_split = 1 forces them)
    R("conv_wgrad", (2, 24, 40, 32, 64), WG + "|wgrad_tn<64,128,0,1>", three=False),
    R("conv_wgrad", (2, 24, 40, 32, 64), WG + "|wgrad_tn_split<64,128,0,1>", tn_split=1),
    R("conv_wgrad", (2, 24, 40, 32, 132), WG + "|wgrad_tn_split<128,128,0,1>"),
    R("conv_wgrad", (3, 12, 20, 4, 132), WG + "|wgrad_tn_split<128,64,0,1>", tn_split=1),
    R("conv_wgrad", (1, 4, 4, 4, 4), WG + "|wgrad_tn_split<64,64,0,1>", tn_split=1),
    # transposed convolution, patch kernels: convt_fwd<tm>, convt_dgrad<..>, convt_wgrad<tn>
    R("convt_fwd", (4, 16, 16, 128, 128), TFW + "|convt_fwd<2>"),
    R("convt_fwd", (2, 8, 16, 96, 64), TFW + "|convt_fwd<4>"),
    R("convt_fwd", (1, 5, 8, 32, 64), TFW + "|convt_fwd<4>"),                           # 8-pixel patch rows, ragged last tile
    R("convt_fwd", (2, 8, 8, 256, 256), TFW + "|convt_fwd<2>"),
    R("convt_fwd", (4, 32, 32, 128, 128), TFW + "|convt_fwd<2>"),
    R("convt_fwd", (2, 48, 48, 256, 128), TFW + "|convt_fwd<2>"),
    R("convt_fwd", (1, 80, 80, 64, 192), TFW + "|convt_fwd<2>"),
    R("convt_fwd", (3, 36, 48, 128, 64), TFW + "|convt_fwd<2>"),
    R("convt_fwd", (5, 30, 32, 192, 64), TFW + "|convt_fwd<2>"),
    R("convt_dgrad", (4, 32, 32, 128, 128), TDG + "|convt_dgrad<2,1,4>"),
    R("convt_dgrad", (4, 32, 32, 128, 128), TDG + "|convt_dgrad<4,1,4>", convt_patch=3),
    R("convt_dgrad", (2, 48, 48, 256, 128), TDG + "|convt_dgrad<2,1,4>"),
    R("convt_dgrad", (1, 80, 80, 64, 192), TDG + "|convt_dgrad<2,2,2>"),
    R("convt_dgrad", (3, 36, 48, 128, 64), TDG + "|convt_dgrad<2,1,4>"),
    R("convt_dgrad", (5, 30, 32, 192, 64), TDG + "|convt_dgrad<2,1,4>"),
    R("convt_dgrad", (1, 65, 70, 64, 128), TDG + "|convt_dgrad<2,2,2>"),               # ragged last pixel tile (M = 4550)
    R("convt_dgrad", (1, 67, 68, 128, 64), TDG + "|convt_dgrad<2,1,4>"),               # ... (M = 4556)
    R("convt_wgrad", (4, 16, 16, 128, 128), TWG + "|convt_wgrad<2>"),
    R("convt_wgrad", (4, 32, 32, 128, 128), TWG + "|convt_wgrad<2>"),
    R("convt_wgrad", (2, 48, 48, 256, 128), TWG + "|convt_wgrad<4>"),
    R("convt_wgrad", (1, 80, 80, 64, 192), TWG + "|convt_wgrad<1>"),
    R("convt_wgrad", (3, 36, 48, 128, 64), TWG + "|convt_wgrad<2>"),
    R("convt_wgrad", (5, 30, 32, 192, 64), TWG + "|convt_wgrad<1>"),
    # ... and the generic kernels on the shapes those refuse.  A forward of K = Cin <= 128 on the row tiles is an exact-f32 kernel
    R("convt_fwd", (1, 65, 70, 64, 128), TFW + "|igemm_nt<64,64,1,1>", three=False),
    R("convt_fwd", (1, 67, 68, 128, 64), TFW + "|igemm_nt<64,64,1,1>", three=False),
    R("convt_fwd", (2, 6, 10, 8, 12), TFW + "|igemm_nt<64,64,1,1>", three=False),
    R("convt_fwd", (2, 6, 10, 160, 36), _nt(TFW, T2, 1, 1)),
    R("convt_fwd", (2, 6, 10, 160, 36), _nt(TFW, T1, 1, 1), nt_tile=1),
    R("convt_fwd", (2, 6, 10, 160, 36), _nt(TFW, T0, 1, 1), nt_tile=0),
    R("convt_dgrad", (4, 16, 16, 128, 128), _nt(TDG, T2, 2, 0)),
    R("convt_dgrad", (2, 8, 8, 256, 256), _nt(TDG, T2, 2, 0)),
    R("convt_dgrad", (2, 6, 10, 8, 12), _nt(TDG, T2, 2, 0)),
    R("convt_dgrad", (1, 5, 8, 32, 64), _nt(TDG, T2, 2, 0)),
    R("convt_dgrad", (2, 6, 10, 160, 36), _nt(TDG, T1, 2, 0), nt_tile=1),
    R("convt_dgrad", (2, 6, 10, 160, 36), _nt(TDG, T0, 2, 0), nt_tile=0),
    R("convt_wgrad", (2, 8, 8, 256, 256), TWG + "|wgrad_tn_split<128,128,1,0>"),
    R("convt_wgrad", (1, 67, 68, 128, 64), TWG + "|wgrad_tn_split<128,128,1,0>"),
    R("convt_wgrad", (1, 65, 70, 64, 128), TWG + "|wgrad_tn<128,64,1,0>", three=False),
    R("convt_wgrad", (1, 65, 70, 64, 128), TWG + "|wgrad_tn_split<128,64,1,0>", tn_split=1),
    R("convt_wgrad", (1, 5, 8, 32, 64), TWG + "|wgrad_tn<128,64,1,0>", three=False),
    R("convt_wgrad", (2, 6, 10, 8, 12), TWG + "|wgrad_tn<64,64,1,0>", three=False),
    R("convt_wgrad", (2, 6, 10, 8, 12), TWG + "|wgrad_tn_split<64,64,1,0>", tn_split=1),
    R("convt_wgrad", (2, 6, 10, 160, 16), TWG + "|wgrad_tn_split<64,128,1,0>", tn_split=1),
    # conv1x1 (bilinear up-mode): 189 pixels, Cin = 160 = 10 chunks
    R("c1_fwd", (3, 7, 9, 160, 72), _nt("conv1x1_fwd", T2, 1, 0)),
    R("c1_fwd", (3, 7, 9, 160, 72), _nt("conv1x1_fwd", T1, 1, 0), nt_tile=1),
    R("c1_fwd", (3, 7, 9, 160, 72), _nt("conv1x1_fwd", T0, 1, 0), nt_tile=0),
    R("c1_dgrad", (3, 7, 9, 160, 72), _nt("conv1x1_dgrad", T2, 1, 0)),
    R("c1_dgrad", (3, 7, 9, 160, 72), _nt("conv1x1_dgrad", T1, 1, 0), nt_tile=1),
    R("c1_dgrad", (3, 7, 9, 160, 72), _nt("conv1x1_dgrad", T0, 1, 0), nt_tile=0),
    R("c1_wgrad", (3, 7, 9, 160, 72), "conv1x1_wgrad|wgrad_tn_split<128,128,0,0>"),
    R("c1_wgrad", (3, 7, 9, 160, 72), "conv1x1_wgrad|wgrad_tn_split<128,64,0,0>", tn_split=1, tn_tile=128064),
    R("c1_wgrad", (3, 7, 9, 160, 72), "conv1x1_wgrad|wgrad_tn_split<64,128,0,0>", tn_split=1, tn_tile=64128),
    R("c1_wgrad", (3, 7, 9, 160, 72), "conv1x1_wgrad|wgrad_tn_split<64,64,0,0>", tn_split=1, tn_tile=64064),
]


def _work(r):
    n, h, w, cin, cout = r.shape
    return n * h * w * cin * cout


def _pos_rows():
    """one all-positive row per kernel class that has a three-product body: the cheapest shape of the class"""
    best = {}
    for r in LEDGER:
        if r.three and (r.cls not in best or _work(r) < _work(best[r.cls])):
            best[r.cls] = r
    return [r._replace(flavour="pos") for r in best.values()]


POS_ROWS = _pos_rows()

# Every class string the three launch sites can print for a SPLIT kernel, over the planner's and the knobs' value ranges:
#   rd_igemm.hip launch_nt: "%s|conv3_halo_split<64,w8>", "%s|conv3_halo_split<%d>" (128 | 64) for the A_CONV3 / EPI_STORE callers
#     (conv3x3_fwd, conv3x3_dgrad); "%s|igemm_nt_split<%s,%d,%d>" with the tile 128,128 | 128,64 | 64,64 and (AMODE, EPI) of the
#     caller: conv3x3_* (0,0), convt2x2_fwd (1,1), convt2x2_dgrad (2,0), conv1x1_* (1,0);
#   rd_igemm.hip launch_tn: "%s|wgrad_tn_split<%d,%d,%d,%d>", bm, bn in {64, 128}, (AMODE, BMODE) = conv3x3_wgrad (0,1),
#     convt2x2_wgrad (1,0), conv1x1_wgrad (0,0);
#   rd_convt.hip: "convt2x2_dgrad|convt_dgrad<4,1,4 | 2,1,4 | 2,2,2>", "convt2x2_wgrad|convt_wgrad<4 | 2 | 1>",
#     "convt2x2_fwd|convt_fwd<2 | 4>";
#   rd_wgrad_strip.hip: "conv3x3_wgrad|wgrad_strip_tr<occ,2,2,w8 | occ,2,2 | occ,4,1>", occ in {1, 2}.
PRINTABLE_SPLIT_CLASSES = (
    [op + "|conv3_halo_split<%s>" % v for op in (FW, DG) for v in ("64,w8", "128", "64")]
    + [_nt(op, t, a, e) for op, a, e in ((FW, 0, 0), (DG, 0, 0), (TFW, 1, 1), (TDG, 2, 0), ("conv1x1_fwd", 1, 0), ("conv1x1_dgrad", 1, 0))
       for t in (T0, T1, T2)]
    + ["%s|wgrad_tn_split<%d,%d,%d,%d>" % (op, bm, bn, a, b) for op, a, b in ((WG, 0, 1), (TWG, 1, 0), ("conv1x1_wgrad", 0, 0))
       for bm in (64, 128) for bn in (64, 128)]
    + [TDG + "|convt_dgrad<%s>" % v for v in ("4,1,4", "2,1,4", "2,2,2")]
    + [TWG + "|convt_wgrad<%d>" % v for v in (4, 2, 1)]
    + [TFW + "|convt_fwd<%d>" % v for v in (2, 4)]
    + [STRIP % ("%d,%s" % (occ, v)) for occ in (1, 2) for v in ("2,2,w8", "2,2", "4,1")])


# ---- operands and fp64 references (CPU), shared between the rows of a shape ---------------------------------------------------
@functools.lru_cache(maxsize=4)
def _operands(base, shape, flavour):
    n, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(1000003 * n + 1009 * h + 101 * w + 13 * cin + cout)
    f = (lambda t: t.abs()) if flavour == "pos" else (lambda t: t)
    up = 2 if base == "convt" else 1
    x = f(torch.randn(n, h, w, cin, generator=g))
    wshape = {"conv": (cout, cin, 3, 3), "convt": (cin, cout, 2, 2), "c1": (cout, cin, 1, 1)}[base]
    wt = f(torch.randn(wshape, generator=g)) * 0.05
    gy = f(torch.randn(n, up * h, up * w, cout, generator=g)) * 1e-5        # gradient-sized: about 2^17 below the activations
    return x, wt, gy


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _quads(g, n, h, w, c):
    """[n, 2h, 2w, c] -> [n*h*w, (a, b, c)]: the four fine pixels of every coarse one"""
    return g.reshape(n, h, 2, w, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n * h * w, 4 * c)


def _op64(fam, shape, a, b):
    """the op of `fam` on fp64 operands (a, b) = (x, w) forward | (gy, w) data gradient | (gy, x) weight gradient"""
    n, h, w, cin, cout = shape
    if fam == "conv_fwd":
        return F.conv2d(_nchw(a), b, None, 1, 1).permute(0, 2, 3, 1)
    if fam == "conv_dgrad":
        return F.conv_transpose2d(_nchw(a), b, None, 1, 1).permute(0, 2, 3, 1)
    if fam == "conv_wgrad":
        unf = F.unfold(_nchw(b), 3, padding=1)                                  # [n, cin * 9, h * w]
        return torch.einsum("npo,nkp->ok", a.reshape(n, h * w, cout), unf).reshape(cout, cin, 3, 3)
    if fam == "convt_fwd":
        o = a.reshape(-1, cin) @ b.permute(0, 2, 3, 1).reshape(cin, 4 * cout)
        return o.reshape(n, h, w, 2, 2, cout).permute(0, 1, 3, 2, 4, 5).reshape(n, 2 * h, 2 * w, cout)
    if fam == "convt_dgrad":
        return (_quads(a, n, h, w, cout) @ b.permute(0, 2, 3, 1).reshape(cin, 4 * cout).t()).reshape(n, h, w, cin)
    if fam == "convt_wgrad":
        return (b.reshape(-1, cin).t() @ _quads(a, n, h, w, cout)).reshape(cin, 2, 2, cout).permute(0, 3, 1, 2)
    if fam == "c1_fwd":
        return (a.reshape(-1, cin) @ b.reshape(cout, cin).t()).reshape(n, h, w, cout)
    if fam == "c1_dgrad":
        return (a.reshape(-1, cout) @ b.reshape(cout, cin)).reshape(n, h, w, cin)
    if fam == "c1_wgrad":
        return (a.reshape(-1, cout).t() @ b.reshape(-1, cin)).reshape(cout, cin, 1, 1)
    raise ValueError(fam)


def _pair(fam, shape, flavour):
    x, wt, gy = _operands(fam.split("_")[0], shape, flavour)
    return {"fwd": (x, wt), "dgrad": (gy, wt), "wgrad": (gy, x)}[fam.split("_")[1]]


@functools.lru_cache(maxsize=2)
def _refs(fam, shape, flavour):
    a, b = (t.double() for t in _pair(fam, shape, flavour))
    return _op64(fam, shape, a, b).contiguous(), _op64(fam, shape, a.abs(), b.abs()).contiguous()


def _prepare(fam, shape, flavour):
    """operands on the device, tagged / packed under the CURRENT mode -> a closure that launches the op under test (only)"""
    from resdepth_amd import ops
    x, wt, gy = _operands(fam.split("_")[0], shape, flavour)
    tg = lambda t: ops.amax_of(t.to(DEV))
    base, kind = fam.split("_")
    if kind == "wgrad":
        xd, gd = tg(x), tg(gy)
        f = {"conv": ops.conv3x3_bwd_weight, "convt": ops.convt2x2_bwd_weight, "c1": ops.conv1x1_bwd_weight}[base]
        return lambda: f(xd, gd)
    pf, pd = {"conv": ops.pack_conv3x3_weight, "convt": ops.pack_convt2x2_weight, "c1": ops.pack_conv1x1_weight}[base](wt.to(DEV))
    if kind == "fwd":
        xd = tg(x)
        if base == "convt":
            return lambda: ops.convt2x2_fwd(xd, pf, None, None)
        return (lambda: ops.conv3x3_fwd(xd, pf)) if base == "conv" else (lambda: ops.conv1x1_fwd(xd, pf))
    gd = tg(gy)
    f = {"conv": ops.conv3x3_bwd_data, "convt": ops.convt2x2_bwd_data, "c1": ops.conv1x1_bwd_data}[base]
    return lambda: f(gd, pd)


def _classes(lib, launch):
    """(result, class strings the MFMA launch sites reported for this launch)"""
    lib.prof_enable(1)
    try:
        lib.prof_reset()
        out = launch()
        torch.cuda.synchronize()
        return out, [e["name"] for e in lib.prof_collect() if e["launches"] > 0]
    finally:
        lib.prof_enable(0)
        lib.prof_reset()


def _run_modes(lib, r):
    """-> out3 (device tensor, slot attached when a producer), its second run, out6, exact, classes"""
    with _knobs(lib, r.knobs):
        with lib.AmaxPool(DEV):
            launch = _prepare(r.fam, r.shape, r.flavour)
            out3, classes = _classes(lib, launch)
            again = launch()
        with _knobs(lib, {"mfma_products": 6}):
            out6 = _prepare(r.fam, r.shape, r.flavour)()
    with _knobs(lib, {"mfma_f32": 1}):
        exact = _prepare(r.fam, r.shape, r.flavour)()
    return out3, again, out6, exact, classes


def _rid(r):
    return "%s-%s-%s%s" % (r.fam, "x".join(map(str, r.shape)), ",".join("%s=%d" % kv for kv in r.knobs) or "auto",
                           "-pos" if r.flavour == "pos" else "")


def _common(lib, r):
    out3, again, out6, exact, classes = _run_modes(lib, r)
    assert classes == [r.cls], (_rid(r), "launched", classes, "the ledger expects", r.cls)
    assert torch.isfinite(out3).all()
    assert torch.equal(out3, again), (_rid(r), "a second run gave other bits")
    if r.three:
        assert not torch.equal(out3, out6), (_rid(r), "the three-product body did not run")
    else:
        assert torch.equal(out3, out6), (_rid(r), "a launch without a split kernel must not depend on the slots")
    if r.fam in ("conv_dgrad", "convt_fwd"):
        assert _slot_max(out3) == float(out3.abs().max()), (_rid(r), _slot_max(out3), float(out3.abs().max()))
    return out3.double().cpu(), exact.double().cpu()


@pytest.mark.parametrize("r", LEDGER, ids=_rid)
def test_ledger_row_runs_its_kernel_on_three_products_within_the_element_bound(lib, r):
    ref, den = _refs(r.fam, r.shape, r.flavour)
    out3, exact = _common(lib, r)
    err = (out3 - ref).abs()
    bound = 16 * U * den + 2.5 * (exact - ref).abs()
    worst = float((err / (U * den)).max())
    print("MARGIN %s | %s | err/(u den) max %.3f | err/bound max %.3f" % (r.cls, _rid(r), worst, float((err / bound).max())))
    assert bool((err <= bound).all()), (_rid(r), "err / bound", float((err / bound).max()), "err / (u den)", worst)


@pytest.mark.parametrize("r", POS_ROWS, ids=_rid)
def test_all_positive_operands_per_kernel_class(lib, r):
    """the `pos` flavour of scripts/split_numerics.py: every product has the same sign, nothing cancels, so an accumulator
    mix-up (hi / lo) cannot hide; tensor-level bars of test_per_op_error_bound_and_below_the_exact_f32_chain"""
    ref, den = _refs(r.fam, r.shape, r.flavour)
    out3, exact = _common(lib, r)
    e = (out3 - ref).abs() / den
    f = (exact - ref).abs() / den
    s_max, s_rms = float(e.max()) / U, float(e.pow(2).mean().sqrt()) / U
    f_max, f_rms = float(f.max()) / U, float(f.pow(2).mean().sqrt()) / U
    print("MARGIN-POS %s | %s | s_max %.3f s_rms %.3f | f_max %.3f f_rms %.3f" % (r.cls, _rid(r), s_max, s_rms, f_max, f_rms))
    assert s_max <= 12.0 + 2.5 * f_max + 4.0, (_rid(r), s_max, f_max)
    assert s_rms <= 1.5 * f_rms + 0.5, (_rid(r), s_rms, f_rms)


@pytest.mark.parametrize("fam,shape", [("conv_fwd", (32, 8, 8, 512, 512)), ("conv_dgrad", (33, 8, 8, 64, 256)),
                                       ("conv_fwd", (33, 8, 8, 256, 64))])
def test_8x8_split_k_and_unsplit_forms_give_the_same_bits_on_three_products(lib, fam, shape):
    """the blocks of a tile park their K range in the scratch slab and the last one adds the ranges in the
    order of the unsplit form, which a stream without the scratch runs -- in mode 3 the parked values are scaled-back
    accumulators of the three-product body"""
    launch = _prepare(fam, shape, "randn")
    split, classes = _classes(lib, launch)
    assert classes[0].endswith("conv3_halo_split<64,w8>")
    side = torch.cuda.Stream()                                    # no rd_set_splitk_workspace registration: unsplit
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        unsplit = launch()
    side.synchronize()
    assert torch.equal(split, unsplit)
    with _knobs(lib, {"mfma_products": 6}):
        assert not torch.equal(split, _prepare(fam, shape, "randn")())


def test_every_printable_split_class_has_a_three_product_row():
    covered = {r.cls for r in LEDGER if r.three}
    missing = [c for c in PRINTABLE_SPLIT_CLASSES if c not in covered]
    assert not missing, missing
    # ... and the ledger names no class the launch sites cannot print (a typo would otherwise only fail on the device)
    unknown = [r.cls for r in LEDGER if r.three and r.cls not in PRINTABLE_SPLIT_CLASSES]
    assert not unknown, unknown
    assert {r.cls for r in POS_ROWS} == covered


# ---- the fused entry points, mode 3 with slots -------------------------------------------------------------------------------
def _close(a, b, tol, name):
    """tests/test_ops_gpu.py `close`: rel-L2 <= tol and max-abs / scale <= 50 tol"""
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    r = float((a - b).norm() / (b.norm() + 1e-30))
    assert r <= tol, "%s: rel-L2 %.3e > %g" % (name, r, tol)
    m = float((a - b).abs().max()) / (float(b.abs().max()) + 1e-30)
    assert m <= 50 * tol, "%s: max-abs/scale %.3e" % (name, m)


def _element_bound(out3, exact, ref, den, name):
    err = (out3.double().cpu() - ref).abs()
    bound = 16 * U * den + 2.5 * (exact.double().cpu() - ref).abs()
    print("MARGIN %s | err/(u den) max %.3f" % (name, float((err / (U * den)).max())))
    assert bool((err <= bound).all()), (name, float((err / bound).max()))


@pytest.mark.parametrize("shape", [(2, 8, 16, 8, 24), (3, 32, 32, 20, 36), (8, 64, 64, 32, 128), (33, 8, 8, 64, 256),
                                   (33, 8, 8, 128, 64)])      # the last one: the two-image form with two K ranges
def test_statistics_epilogues_see_the_scaled_back_accumulators(lib, shape):
    """rd_conv3x3_fwd_stats / rd_conv3x3_fwd_bn: the three-product accumulators hold the products of the SCALED operands; sums,
    mean, invstd and the running statistics must be those of the z the kernel stored"""
    from resdepth_amd import ops
    n, h, w, cin, cout = shape
    x, wt, _ = _operands("conv", shape, "randn")
    ref, den = _refs("conv_fwd", shape, "randn")
    wf, _ = ops.pack_conv3x3_weight(wt.to(DEV))
    xd = ops.amax_of(x.to(DEV))
    z, sums = ops.conv3x3_fwd_stats(xd, wf)
    assert torch.equal(z, ops.conv3x3_fwd(xd, wf))
    with _knobs(lib, {"mfma_products": 6}):
        assert not torch.equal(z, _prepare("conv_fwd", shape, "randn")()), "the three-product body did not run"
    with _knobs(lib, {"mfma_f32": 1}):
        exact = _prepare("conv_fwd", shape, "randn")()
    _element_bound(z, exact, ref, den, "fwd_stats z %s" % (shape,))
    zz = z.double().reshape(-1, cout)
    _close(sums[:cout], zz.sum(0), 1e-6, "sum")
    _close(sums[cout:], (zz * zz).sum(0), 1e-6, "sumsq")
    rm = torch.linspace(-1, 1, cout, device=DEV)
    rv = torch.linspace(0.5, 2, cout, device=DEV)
    rm0, rv0 = rm.double(), rv.double()
    nbt = torch.tensor(7, device=DEV)
    zf, mean, invstd = ops.conv3x3_fwd_bn(xd, wf, rm, rv, nbt)
    assert torch.equal(zf, z) and int(nbt) == 8
    count = n * h * w
    m64 = zz.mean(0)
    v64 = (zz * zz).mean(0) - m64 * m64
    _close(mean, m64, 1e-6, "mean")
    _close(invstd, (v64 + ops.BN_EPS).rsqrt(), 1e-6, "invstd")
    _close(rm, (1 - ops.BN_MOMENTUM) * rm0 + ops.BN_MOMENTUM * m64, 1e-6, "running mean")
    _close(rv, (1 - ops.BN_MOMENTUM) * rv0 + ops.BN_MOMENTUM * v64 * count / (count - 1), 1e-6, "running var")


def _hook_sums64(z, mean, invstd, gamma, beta, slope, g, mode):
    """fp64 form of rd_bn_act_bwd_reduce over the hook's block: sum g', sum g' xhat, sum g (mode 1), sum_{y <= 0} g y"""
    c = z.shape[-1]
    z, g = z.double().reshape(-1, c), g.double().reshape(-1, c)
    xhat = (z - mean.double()) * invstd.double()
    y = xhat * gamma.double() + beta.double()
    gp = torch.where(y > 0, g, slope * g)
    neg = torch.where(y > 0, torch.zeros_like(g), g * y)
    s2 = g.sum(0) if mode == 1 else torch.zeros(c, dtype=torch.float64, device=z.device)
    return torch.cat([gp.sum(0), (gp * xhat).sum(0), s2, neg.sum(0)])


@pytest.mark.parametrize("n,h,w,cin,cout,mode,kind", [
    (2, 32, 32, 64, 128, 1, "conv"), (8, 64, 64, 64, 128, 1, "conv"), (16, 64, 64, 128, 256, 2, "conv"), (2, 16, 16, 20, 36, 1, "conv"),
    (3, 24, 40, 32, 64, 1, "conv"), (2, 48, 80, 64, 128, 2, "conv"), (32, 8, 8, 512, 512, 1, "conv"), (33, 8, 8, 256, 64, 2, "conv"),
    (4, 16, 16, 128, 128, 1, "convt"), (2, 8, 8, 256, 256, 1, "convt"), (2, 6, 10, 8, 12, 1, "convt"), (4, 32, 32, 128, 128, 1, "convt"),
    (2, 48, 48, 256, 128, 1, "convt"), (1, 80, 80, 64, 192, 1, "convt"),
    (1, 65, 70, 64, 128, 1, "convt"),       # a ragged last pixel tile of convt_dgrad<2,2,2> (M = 4550)
    (3, 12, 20, 8, 24, 1, "conv")])         # ... and of the generic row tiles (M = 720 = 11.25 tiles)
def test_bn_backward_hook_sums_from_three_product_data_gradients(lib, n, h, w, cin, cout, mode, kind):
    """rd_conv3x3_bwd_data_bnstats / rd_convt2x2_bwd_data_bnstats (shapes of tests/test_ops_gpu.py
    test_bn_backward_statistics_from_the_data_gradient_epilogues + two ragged pixel tiles): dx on the element bound, bit-identical
    to the plain entry point, and the four sums of the hook, after rd_bn_bwd_stats_finalize, against fp64 over the kernel's own
    dx at that test's tolerance (1e-5 of the largest channel sum of each kind)."""
    from resdepth_amd import ops
    shape = (n, h, w, cin, cout)
    fam = "conv_dgrad" if kind == "conv" else "convt_dgrad"
    _, wt, gy = _operands(kind, shape, "randn")
    g = torch.Generator().manual_seed(n * 1000 + h * 10 + cin)
    C = cin
    zb = torch.randn(n, h, w, C, generator=g).to(DEV)
    mean, invstd = (torch.randn(C, generator=g) * 0.1).to(DEV), (torch.rand(C, generator=g) + 0.5).to(DEV)
    gamma, beta = torch.randn(C, generator=g).to(DEV), (torch.randn(C, generator=g) * 0.3).to(DEV)
    pack, op = (ops.pack_conv3x3_weight, ops.conv3x3_bwd_data) if kind == "conv" else (ops.pack_convt2x2_weight, ops.convt2x2_bwd_data)
    _, wd = pack(wt.to(DEV))
    gd = ops.amax_of(gy.to(DEV))
    hook = ops.BnHook(zb, mean, invstd, gamma, beta, 0.01, None, mode if kind == "conv" else 1)
    with lib.AmaxPool(DEV):
        dx, part = op(gd, wd, bn=hook)
        plain = op(gd, wd)
    assert torch.equal(dx, plain) and part[1] > 0
    if kind == "conv":
        assert _slot_max(dx) == float(dx.abs().max())
    with _knobs(lib, {"mfma_products": 6}):
        assert not torch.equal(dx, _prepare(fam, shape, "randn")()), "the three-product body did not run"
    with _knobs(lib, {"mfma_f32": 1}):
        exact = _prepare(fam, shape, "randn")()
    ref, den = _refs(fam, shape, "randn")
    _element_bound(dx, exact, ref, den, "bnstats dx %s %s" % (kind, shape))
    sums = ops.bn_bwd_stats_finalize([part], C)
    want = _hook_sums64(zb, mean, invstd, gamma, beta, 0.01, dx, hook.mode)
    scale = want.abs().view(4, C).amax(1, keepdim=True).expand(4, C).reshape(-1) + 1e-30
    assert float(((sums - want).abs() / scale).max()) <= 1e-5


@pytest.mark.parametrize("slope", [0.0, 0.01])
@pytest.mark.parametrize("shape", [(4, 16, 16, 128, 128), (2, 6, 10, 160, 36)])      # convt_fwd<2> | generic row tiles, ragged
def test_convt_fwd_bnskip_on_three_products(lib, shape, slope):
    """rd_convt2x2_fwd_bnskip against fp64 convT + bias + act(BN(z_skip)).  den: the contraction's sum |x| |w| plus the
    magnitudes of the terms the epilogue adds in fp32 (bias, and the BN expression's own operands: its few roundings are also in
    `exact`, the same entry point on the exact-f32 kernels)."""
    from resdepth_amd import ops
    n, h, w, cin, cout = shape
    x, wt, _ = _operands("convt", shape, "randn")
    g = torch.Generator().manual_seed(cin + cout)
    bias = torch.randn(cout, generator=g)
    zs = torch.randn(n, 2 * h, 2 * w, cout, generator=g) * 2
    mean, invstd = torch.randn(cout, generator=g) * 0.1, torch.rand(cout, generator=g) + 0.5
    gamma, beta = torch.randn(cout, generator=g), torch.randn(cout, generator=g) * 0.3
    conv, cden = _refs("convt_fwd", shape, "randn")
    y = (zs.double() - mean.double()) * invstd.double() * gamma.double() + beta.double()
    ref = conv + bias.double() + torch.where(y > 0, y, slope * y)
    den = cden + bias.abs().double() + (zs.abs().double() + mean.abs().double()) * invstd.double() * gamma.abs().double() + beta.abs().double()
    args = [t.to(DEV) for t in (bias, zs, mean, invstd, gamma, beta)]

    def run():
        wtf, _ = ops.pack_convt2x2_weight(wt.to(DEV))
        with lib.AmaxPool(DEV):
            return ops.convt2x2_fwd_bnskip(ops.amax_of(x.to(DEV)), wtf, *args, slope)
    out3 = run()
    assert torch.equal(out3, run())
    assert _slot_max(out3) == float(out3.abs().max())
    with _knobs(lib, {"mfma_products": 6}):
        assert not torch.equal(out3, run()), "the three-product body did not run"
    with _knobs(lib, {"mfma_f32": 1}):
        exact = run()
    _element_bound(out3, exact, ref, den, "bnskip %s slope %g" % (shape, slope))


def _fwd_act_case(shape, seed):
    n, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, cin, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * 0.05
    scale = torch.rand(cout, generator=g) + 0.5
    shift = torch.randn(cout, generator=g) * 0.2
    return x, wt, scale, shift


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("shape", [(3, 16, 48, 64, 64), (2, 16, 32, 64, 128)])
def test_folded_inference_convolution_on_three_products(lib, shape, pool):
    """rd_conv3x3_fwd_act, per-tensor slots: a = act(conv(x, w * scale) + shift) against fp64 of the same folded fp32 weights
    (one IEEE multiply: the host's product is the packer's), the pooled output = the 2 x 2 maxima of the kernel's own a, both out
    slots exact.  exact = the exact-f32 convolution of the folded weights + shift + activation (the entry point itself exists in
    the split kernels only); the activation is 1-Lipschitz, so the element bound of the contraction carries over."""
    from resdepth_amd import ops
    n, h, w, cin, cout = shape
    slope = 0.01
    x, wt, scale, shift = _fwd_act_case(shape, 31 + cout + int(pool))
    wfold = wt * scale.view(-1, 1, 1, 1)
    act = lambda v: torch.where(v > 0, v, slope * v)
    ref = act(F.conv2d(_nchw(x).double(), wfold.double(), None, 1, 1).permute(0, 2, 3, 1) + shift.double())
    den = F.conv2d(_nchw(x).double().abs(), wfold.double().abs(), None, 1, 1).permute(0, 2, 3, 1) + shift.abs().double()

    def run():
        wff = ops.pack_conv3x3_weight_folded(wt.to(DEV), scale.to(DEV))
        with lib.AmaxPool(DEV):
            return ops.conv3x3_fwd_act(ops.amax_of(x.to(DEV)), wff, shift.to(DEV), slope, pool=pool)
    a, p = run()
    a2, p2 = run()
    assert torch.equal(a, a2) and (p is None) == (not pool) and (p is None or torch.equal(p, p2))
    assert _slot_max(a) == float(a.abs().max())
    if pool:
        assert torch.equal(p, F.max_pool2d(_nchw(a), 2, 2).permute(0, 2, 3, 1))
        assert _slot_max(p) == float(p.abs().max())
    with _knobs(lib, {"mfma_products": 6}):
        assert not torch.equal(a, run()[0]), "the three-product body did not run"
    with _knobs(lib, {"mfma_f32": 1}):
        wf32, _ = ops.pack_conv3x3_weight(wfold.to(DEV), need_dgrad=False)
        exact = act(ops.conv3x3_fwd(x.to(DEV), wf32) + shift.to(DEV))
    _element_bound(a, exact, ref, den, "fwd_act %s pool %d" % (shape, pool))


def _per_image_slots(lib, pool, x):
    """tag x with a slot ARRAY from a per-image pool, every image's slot computed by rd_amax over that image"""
    from resdepth_amd import ops
    slots = pool.take()
    for i in range(x.shape[0]):
        lib.check(lib.load().rd_amax(x[i].data_ptr(), x[i].numel(), slots[i * lib.AMAX_WORDS:].data_ptr(), lib.stream_ptr()), "amax")
    return lib.tag(x, slots)


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("shape", [(3, 16, 48, 64, 64), (3, 16, 32, 64, 128)])
def test_folded_inference_convolution_with_per_image_slots(lib, shape, pool):
    """AmaxPool(per_image=3), image 1 scaled x 300: every image's result is bit-identical to the image run alone (its own
    scale, not the batch's), every image's slot holds that image's own maximum, and the three-product body ran"""
    from resdepth_amd import ops
    n, h, w, cin, cout = shape
    x, wt, scale, shift = _fwd_act_case(shape, 77 + cout)
    x[1] *= 300.0
    xd = x.to(DEV)
    wff = ops.pack_conv3x3_weight_folded(wt.to(DEV), scale.to(DEV))
    sh = shift.to(DEV)

    def run(xs):
        with lib.AmaxPool(DEV, per_image=xs.shape[0]) as pl:
            return ops.conv3x3_fwd_act(_per_image_slots(lib, pl, xs.contiguous()), wff, sh, 0.01, pool=pool)
    a, p = run(xd)
    for out in (a, p) if pool else (a,):
        sl = lib.slot_of(out).view(n, 16, 32)[:, :, 0].max(dim=1).values.contiguous().view(torch.float32)
        assert torch.equal(sl, out.abs().amax(dim=(1, 2, 3)))
    for i in range(n):
        ai, pi = run(xd[i:i + 1])
        assert torch.equal(ai[0], a[i]), i
        assert not pool or torch.equal(pi[0], p[i]), i
    six, _ = ops.conv3x3_fwd_act(xd.clone(), wff, sh, 0.01, pool=pool)       # an untagged copy: six products
    assert not torch.equal(six, a), "the three-product body did not run"
    assert float((six - a).abs().max()) <= 2e-5 * float(six.abs().max())


@pytest.mark.parametrize("n,h,w,cin,cout", [(16, 64, 64, 128, 256), (8, 64, 64, 128, 64), (33, 8, 8, 256, 64), (4, 16, 16, 64, 64)])
def test_staged_epilogues_equal_the_register_direct_ones_on_three_products(lib, n, h, w, cin, cout):
    """nt_epi = 0 in mode 3 (shapes of tests/test_ops_gpu.py test_register_direct_epilogues_equal_the_staged_ones): the scale-back
    happens before either epilogue, so z, dx, the folded activation and the pooled values are the same bits"""
    from resdepth_amd import ops
    g = torch.Generator().manual_seed(n + h + cin + cout)
    x = torch.randn(n, h, w, cin, generator=g).to(DEV)
    dz = (torch.randn(n, h, w, cout, generator=g) * 1e-5).to(DEV)
    wt = (torch.randn(cout, cin, 3, 3, generator=g) * 0.05).to(DEV)
    scale = (torch.rand(cout, generator=g) + 0.5).to(DEV)
    shift = (torch.randn(cout, generator=g) * 0.2).to(DEV)
    pool = w % 16 == 0 and h % 8 == 0 and w > 8

    def run():
        wf, wd = ops.pack_conv3x3_weight(wt)
        wfold = ops.pack_conv3x3_weight_folded(wt, scale)
        xd, gd = ops.amax_of(x.clone()), ops.amax_of(dz.clone())
        with lib.AmaxPool(DEV):
            z, sums = ops.conv3x3_fwd_stats(xd, wf)
            dx = ops.conv3x3_bwd_data(gd, wd)
            a, p = ops.conv3x3_fwd_act(xd, wfold, shift, 0.01, pool=pool)
        return z, sums, dx, a, p
    with _knobs(lib, {"nt_epi": 0}):
        z0, s0, dx0, a0, p0 = run()
    z1, s1, dx1, a1, p1 = run()
    with _knobs(lib, {"mfma_products": 6}):
        z6 = run()[0]
    assert not torch.equal(z1, z6), "the three-product body did not run"
    assert torch.equal(z0, z1) and torch.equal(dx0, dx1) and torch.equal(a0, a1)
    assert (p0 is None) == (p1 is None) and (p0 is None or torch.equal(p0, p1))
    assert _slot_max(dx0) == _slot_max(dx1) == float(dx1.abs().max())
    _close(s1, s0, 1e-6, "BN statistics")
