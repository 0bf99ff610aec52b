"""Restatements of the level-0 operations (first convolution, last convolution, the first block's BatchNorm + activation +
pool and its backward, the composed tail) written from the mathematics and from lib/UNet.py's layer sequence with plain torch
CPU ops -- shifted slices and einsum, no convolution primitive, nothing ported from the kernels.

Every function takes `dtype`: torch.float64 is the reference proper; torch.float32 runs the SAME restatement in fp32 on the
CPU, which is how the tests measure what fp32 arithmetic costs on the inputs at hand (e32 in test_level0_matrix_gpu.py).

Functions that end in a dot product also return its magnitude sum  mag = sum |a| |b|  per output element (bias and
residual terms included with their absolute value): the element-wise error bound of any fp32 summation order is
(n + 2) * 2^-24 * mag for n terms.

Layouts are the library's: activations NHWC [N, H, W, C], the network input NCHW [N, Cin, H, W], the network output and its
gradient [N, 1, H, W]; weights keep torch's layouts (Conv2d [Cout, Cin, 3, 3], ConvTranspose2d [Cin, Cout, 2, 2]).
"""
import torch
import torch.nn.functional as F

F64 = torch.float64


def _c(t, dtype):
    return None if t is None else t.detach().cpu().to(dtype)


def _pad_nchw(x):
    return F.pad(x, (1, 1, 1, 1))


def _pad_nhwc(s):
    return F.pad(s, (0, 0, 1, 1, 1, 1))


# ---- first convolution: z[n, y, x, o] = sum_{c, ky, kx} x[n, c, y + ky - 1, x + kx - 1] w[o, c, ky, kx] -------------------------
def _first_fwd(x, w):
    n, cin, h, wd = x.shape
    xp = _pad_nchw(x)
    z = torch.zeros(n, h, wd, w.shape[0], dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            z += torch.einsum("nchw,oc->nhwo", xp[:, :, ky:ky + h, kx:kx + wd], w[:, :, ky, kx])
    return z


def first_fwd(x, w, dtype=F64):
    """-> (z [N, H, W, Cout], mag)"""
    x, w = _c(x, dtype), _c(w, dtype)
    return _first_fwd(x, w), _first_fwd(x.abs(), w.abs())


def _first_wgrad(x, dz):
    n, cin, h, wd = x.shape
    xp = _pad_nchw(x)
    dw = torch.zeros(dz.shape[3], cin, 3, 3, dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = torch.einsum("nchw,nhwo->oc", xp[:, :, ky:ky + h, kx:kx + wd], dz)
    return dw


def first_wgrad(x, dz, dtype=F64):
    """dw[o, c, ky, kx] = sum_{n, y, x} x[n, c, y + ky - 1, x + kx - 1] dz[n, y, x, o] -> (dw [Cout, Cin, 3, 3], mag)"""
    x, dz = _c(x, dtype), _c(dz, dtype)
    return _first_wgrad(x, dz), _first_wgrad(x.abs(), dz.abs())


# ---- last convolution C -> 1 with the outer residual: out = x[:, 0:1] + conv(s, w) + b ----------------------------------------
def _last_conv(s, w):
    n, h, wd, c = s.shape
    sp = _pad_nhwc(s)
    out = torch.zeros(n, h, wd, dtype=s.dtype)
    for ky in range(3):
        for kx in range(3):
            out += torch.einsum("nhwc,c->nhw", sp[:, ky:ky + h, kx:kx + wd], w[0, :, ky, kx])
    return out


def last_fwd(s, w, bias=None, x_nchw=None, dtype=F64):
    """-> (out [N, 1, H, W], mag)"""
    s, w, bias, x_nchw = _c(s, dtype), _c(w, dtype), _c(bias, dtype), _c(x_nchw, dtype)
    out, mag = _last_conv(s, w), _last_conv(s.abs(), w.abs())
    if bias is not None:
        out, mag = out + bias[0], mag + bias[0].abs()
    if x_nchw is not None:
        out, mag = out + x_nchw[:, 0], mag + x_nchw[:, 0].abs()
    return out.unsqueeze(1), mag.unsqueeze(1)


def _last_dgrad(dout, w):
    n, _, h, wd = dout.shape
    dp = F.pad(dout[:, 0], (1, 1, 1, 1))
    ds = torch.zeros(n, h, wd, w.shape[1], dtype=dout.dtype)
    for ky in range(3):
        for kx in range(3):     # s[y + ky - 1, x + kx - 1] fed out[y, x]  =>  ds[q] takes dout[q - (ky - 1, kx - 1)]
            ds += dp[:, 2 - ky:2 - ky + h, 2 - kx:2 - kx + wd].unsqueeze(-1) * w[0, :, ky, kx]
    return ds


def last_dgrad(dout, w, dtype=F64):
    """ds[n, y, x, c] = sum_tap dout[n, 0, y - ky + 1, x - kx + 1] w[0, c, ky, kx] -> (ds [N, H, W, C], mag).  With a 1-channel
    dout this is also the `LastConvGrad` operand: the full-resolution gradient that enters the first block's backward."""
    dout, w = _c(dout, dtype), _c(w, dtype)
    return _last_dgrad(dout, w), _last_dgrad(dout.abs(), w.abs())


def _last_wgrad(s, dout):
    n, h, wd, c = s.shape
    sp = _pad_nhwc(s)
    dw = torch.zeros(1, c, 3, 3, dtype=s.dtype)
    for ky in range(3):
        for kx in range(3):
            dw[0, :, ky, kx] = torch.einsum("nhwc,nhw->c", sp[:, ky:ky + h, kx:kx + wd], dout[:, 0])
    return dw


def last_wgrad(s, dout, dtype=F64):
    """-> (dw [1, C, 3, 3], dbias [1], mag of dw, mag of dbias)"""
    s, dout = _c(s, dtype), _c(dout, dtype)
    return _last_wgrad(s, dout), dout.sum().reshape(1), _last_wgrad(s.abs(), dout.abs()), dout.abs().sum().reshape(1)


# ---- BatchNorm statistics ---------------------------------------------------------------------------------------------------
def bn_stats(z, eps=1e-5, dtype=F64):
    """-> (mean, biased variance, invstd) per channel of z [N, H, W, C]"""
    z = _c(z, dtype)
    zz = z.reshape(-1, z.shape[-1])
    mean = zz.mean(0)
    var = ((zz - mean) ** 2).mean(0)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def bn_running_update(running_mean, running_var, mean, var, count, momentum=0.1, dtype=F64):
    """nn.BatchNorm2d in training mode: the running variance takes the UNBIASED batch variance"""
    rm, rv = _c(running_mean, dtype), _c(running_var, dtype)
    return (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * var * (count / (count - 1.0))


# ---- the first block: BatchNorm + (leaky / P)ReLU + MaxPool2d(2, 2) ---------------------------------------------------------
def _windows(a):
    """[N, H, W, C] -> [N, H/2, W/2, C, 4]: the 2 x 2 window of every pooled pixel, positions in row-major order"""
    n, h, w, c = a.shape
    return a.reshape(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)


def _unwindow(v):
    n, h2, w2, c, _ = v.shape
    return v.reshape(n, h2, w2, c, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(n, 2 * h2, 2 * w2, c)


def bn_act_pool_fwd(z, mean, invstd, gamma, beta, slope, pool=True, dtype=F64):
    """-> (a, pooled | None, idx | None); idx: position 0..3 of the FIRST maximum of the window in row-major order (torch's
    MaxPool2d), uint8"""
    z, mean, invstd, gamma, beta = (_c(t, dtype) for t in (z, mean, invstd, gamma, beta))
    y = (z - mean) * (invstd * gamma) + beta
    a = torch.where(y > 0, y, y * float(slope))
    if not pool:
        return a, None, None
    win = _windows(a)
    pooled = win.amax(-1)
    first = torch.full(pooled.shape, 3, dtype=torch.uint8)
    for k in (2, 1, 0):                                                     # the earliest position that holds the maximum
        first = torch.where(win[..., k] == pooled, torch.full_like(first, k), first)
    return a, pooled, first


def bn_act_bwd(z, mean, invstd, gamma, beta, slope, g_full, g_pool, idx, count, training=True, dtype=F64):
    """The backward of y = gamma (z - mean) invstd + beta, a = act(y), p = maxpool(a) given dL/da = g_full and dL/dp = g_pool
    (either may be None) -> dict(dz, dgamma, dbeta, dslope, sum_g_full, sums [4, C]).
    training: mean / invstd are the batch statistics of z over `count` pixels and the gradient flows through them;
    eval: they are constants."""
    z, mean, invstd, gamma, beta, g_full, g_pool = (_c(t, dtype) for t in (z, mean, invstd, gamma, beta, g_full, g_pool))
    xh = (z - mean) * invstd
    y = xh * gamma + beta
    g = torch.zeros_like(z) if g_full is None else g_full.clone()
    if g_pool is not None:
        onehot = idx.cpu().long().unsqueeze(-1) == torch.arange(4).view(1, 1, 1, 1, 4)
        g = g + _unwindow(onehot.to(dtype) * g_pool.unsqueeze(-1))
    gy = g * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, float(slope)))      # dL/dy
    c = z.shape[-1]
    dbeta = gy.reshape(-1, c).sum(0)
    dgamma = (gy * xh).reshape(-1, c).sum(0)
    dslope = torch.where(y > 0, torch.zeros_like(y), g * y).reshape(-1, c).sum(0)
    sum_gf = (torch.zeros_like(z) if g_full is None else g_full).reshape(-1, c).sum(0)
    if training:
        dz = gamma * invstd * (gy - dbeta / count - xh * (dgamma / count))
    else:
        dz = gamma * invstd * gy
    return dict(dz=dz, dgamma=dgamma, dbeta=dbeta, dslope=dslope, sum_g_full=sum_gf,
                sums=torch.stack([dbeta, dgamma, sum_gf, dslope]))


def first_wgrad_of_block_backward(x, z, mean, invstd, gamma, beta, slope, g_full, g_pool, idx, count, training=True, dout=None,
                                  w_last=None, dtype=F64):
    """The composite the fused kernel evaluates: the first convolution's weight gradient of the block's dz.  With dout / w_last
    the full-resolution operand is the last convolution's data gradient (LastConvGrad) instead of g_full.
    -> (dw, the backward's dict)"""
    if dout is not None:
        g_full = last_dgrad(dout, w_last, dtype)[0]
    b = bn_act_bwd(z, mean, invstd, gamma, beta, slope, g_full, g_pool, idx, count, training, dtype)
    return _first_wgrad(_c(x, dtype), b["dz"]), b


# ---- the tail, un-composed: ConvTranspose2d(k = 2, s = 2) -> skip add -> 3 x 3 convolution to one channel ----------------------
def convt2x2(xc, wt, bt=None, dtype=F64):
    """up[n, 2 i + a, 2 j + b, o] = sum_c xc[n, i, j, c] wt[c, o, a, b] + bt[o];  xc [N, h, w, Cin] -> [N, 2 h, 2 w, C0]"""
    xc, wt, bt = _c(xc, dtype), _c(wt, dtype), _c(bt, dtype)
    n, h, w, _ = xc.shape
    up = torch.einsum("nijc,coab->niajbo", xc, wt).reshape(n, 2 * h, 2 * w, wt.shape[1])
    return up if bt is None else up + bt


def tail_forward(xc, wt, bt, a0, w_last, b_last, x_nchw, dtype=F64):
    """s = convt(xc) + a0 (the skip: act(BN(z)) of level 0); out = x[:, 0:1] + conv(s, w_last) + b_last -> (out, s)"""
    s = convt2x2(xc, wt, bt, dtype) + _c(a0, dtype)
    return last_fwd(s, w_last, b_last, x_nchw, dtype)[0], s


def tail_backward(xc, s, wt, w_last, dout, dtype=F64):
    """Given dL/dout: g = dL/ds (the last convolution's data gradient), then the transposed convolution's two gradients and the
    last convolution's -> dict(g, dxc [N, h, w, Cin], dwt [Cin, C0, 2, 2], dw_last, db_last)"""
    xc, wt = _c(xc, dtype), _c(wt, dtype)
    g = last_dgrad(dout, w_last, dtype)[0]
    n, h, w, cin = xc.shape
    g6 = g.reshape(n, h, 2, w, 2, g.shape[-1])
    dxc = torch.einsum("niajbo,coab->nijc", g6, wt)
    dwt = torch.einsum("nijc,niajbo->coab", xc, g6)
    dwl, dbl, _, _ = last_wgrad(s, dout, dtype)
    return dict(g=g, dxc=dxc, dwt=dwt, dw_last=dwl, db_last=dbl)


# ---- the cases of the exact-integer matrix (shared by the GPU tests and the CPU check of their premise) -----------------------
FIRST_PAIRS = [(cin, cout) for cin in (1, 2, 3, 4) for cout in (32, 64, 128)]      # the segment kernels' instantiations
GENERIC_FIRST_PAIRS = [(5, 64), (3, 48), (6, 32)]                                   # conv_first_kernel<CI> only
LAST_WIDTHS = [16, 32, 64, 20]                                                      # tile kernels; 20: the generic ones
# (N, H, W): one 16 x 32 tile exactly, ragged both ways, smaller than a tile, odd sizes, several images
SPATIAL = [(1, 16, 32), (1, 18, 34), (1, 2, 2), (2, 6, 10), (1, 7, 9), (1, 17, 33), (3, 17, 33)]
# more 16 x 32 tiles than the 1024 persistent blocks: tiny images, and several ragged tiles per image
LOOP_SHAPES = [(1100, 2, 2), (260, 17, 33)]
TILE_H, TILE_W, MAX_BLOCKS = 16, 32, 1024


def tiles(n, h, w):
    return n * -(-h // TILE_H) * -(-w // TILE_W)


def small_ints(shape, gen):
    """integers in [-3, 3] as fp32: every product and partial sum of the cases above is an integer far below 2^24"""
    return torch.randint(-3, 4, shape, generator=gen).float()


def int_first_case(n, h, w, cin, cout):
    g = torch.Generator().manual_seed(1000003 * cin + 1009 * cout + 101 * h + 7 * w + n)
    x, wt, dz = small_ints((n, cin, h, w), g), small_ints((cout, cin, 3, 3), g), small_ints((n, h, w, cout), g)
    z, zmag = first_fwd(x, wt)
    dw, dwmag = first_wgrad(x, dz)
    return dict(x=x, w=wt, dz=dz, z=z, dw=dw, max_mag=float(max(zmag.max(), dwmag.max())))


def int_last_case(n, h, w, c, xc, bias):
    g = torch.Generator().manual_seed(7919 * c + 101 * h + 7 * w + n + 13 * xc + int(bias))
    s, wt, dout = small_ints((n, h, w, c), g), small_ints((1, c, 3, 3), g), small_ints((n, 1, h, w), g)
    b = small_ints((1,), g) if bias else None
    x = small_ints((n, xc, h, w), g)
    out, omag = last_fwd(s, wt, b, x)
    ds, dsmag = last_dgrad(dout, wt)
    dw, db, dwmag, dbmag = last_wgrad(s, dout)
    return dict(s=s, w=wt, dout=dout, b=b, x=x, out=out, ds=ds, dw=dw, db=db,
                max_mag=float(max(omag.max(), dsmag.max(), dwmag.max(), dbmag.max())))
