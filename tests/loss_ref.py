"""Oracle of the masked training losses (resdepth_amd.masked_loss), written from their definition (include/resdepth_hip_loss.h,
DESIGN.md section 3.9), on the host.

The residual r and every decision taken on it are computed in fp32 with the kernels' roundings -- torch CPU fp32 `*`, `+`, `-`
as separate ops round once each, which is what __fmul_rn / __fadd_rn / the subtraction do -- so the oracle and the kernels hold
bit-identical r: the sign of r, the Huber branch and the sign of every neighbour difference are the same in both, and no pixel
needs to be excluded near a kink.  Everything after r is float64.
"""
import torch

KINDS = ("l1", "l2", "huber", "smooth_l1")


def residual(y_pred, y, mean, std):
    """r = fl(fl(fl(yp * std) + mean) - fl(fl(y * std) + mean)) in fp32, [N,1,H,W] on the host."""
    yp = y_pred.detach().cpu().to(torch.float32)
    yt = y.detach().cpu().to(torch.float32)
    n = yp.shape[0]
    sd = std.detach().cpu().to(torch.float32).reshape(n, 1, 1, 1)
    mu = mean.detach().cpu().to(torch.float32).reshape(n, 1, 1, 1)
    p = yp * sd
    p = p + mu
    t = yt * sd
    t = t + mu
    return p - t


def rho_and_slope(r64, kind, delta):
    """rho(r), rho'(r) in float64; sign(0) = 0."""
    a, sg = r64.abs(), torch.sign(r64)
    if kind == "l1":
        return a, sg
    if kind == "l2":
        return r64 * r64, 2.0 * r64
    if kind == "smooth_l1" and delta == 0.0:
        return a, sg
    assert kind in ("huber", "smooth_l1") and delta > 0.0
    quad = a <= delta
    rho = torch.where(quad, 0.5 * r64 * r64, delta * (a - 0.5 * delta))
    d = torch.where(quad, r64, delta * sg)
    if kind == "smooth_l1":
        rho, d = rho / delta, d / delta
    return rho, d


def pair_terms(r, m):
    """S (float64), Q (int) and the integer stencil k [N,1,H,W] of the valid horizontal and vertical neighbour pairs:
    r fp32, m bool.  Differences are ONE fp32 subtraction."""
    k = torch.zeros(r.shape, dtype=torch.int64)
    S, Q = 0.0, 0
    # horizontal: a = (i, j), b = (i, j + 1)
    d = r[..., :, :-1] - r[..., :, 1:]
    v = m[..., :, :-1] & m[..., :, 1:]
    S += float((d.double().abs() * v).sum())
    Q += int(v.sum())
    s = torch.sign(d).to(torch.int64) * v
    k[..., :, :-1] += s
    k[..., :, 1:] -= s
    # vertical: a = (i, j), b = (i + 1, j)
    d = r[..., :-1, :] - r[..., 1:, :]
    v = m[..., :-1, :] & m[..., 1:, :]
    S += float((d.double().abs() * v).sum())
    Q += int(v.sum())
    s = torch.sign(d).to(torch.int64) * v
    k[..., :-1, :] += s
    k[..., 1:, :] -= s
    return S, Q, k


def masked_loss_oracle(y_pred, y, mask, mean, std, kind="l1", delta=1.0, slope_weight=0.0, gout=1.0):
    """-> dict(loss, mae: python floats; g_data, g_slope: float64 [N,1,H,W], the two parts of d loss / d y_pred times gout;
    A, C, D, S, Q, k)."""
    r = residual(y_pred, y, mean, std)
    assert r.dim() == 4 and r.shape[1] == 1
    n = r.shape[0]
    m = mask.detach().cpu().reshape(r.shape) != 0
    m64, r64 = m.double(), r.double()
    sd = std.detach().cpu().to(torch.float32).double().reshape(n, 1, 1, 1)
    rho, drho = rho_and_slope(r64, kind, float(delta))
    A, C, D = float((m64 * r64.abs()).sum()), float(m64.sum()), float((m64 * rho).sum())
    S, Q, k = pair_terms(r, m)
    k = k * m
    lam = float(slope_weight)
    with_slope = lam > 0.0 and Q > 0
    loss = D / C + (lam * S / Q if with_slope else 0.0)
    g_data = gout * sd * m64 * drho / C
    g_slope = gout * sd * (lam / Q) * k.double() if with_slope else torch.zeros_like(g_data)
    return dict(loss=loss, mae=A / C, g_data=g_data, g_slope=g_slope, A=A, C=C, D=D, S=S, Q=Q, k=k, r=r, m=m)
