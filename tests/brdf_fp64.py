"""Plain restatements of the `--model_name none` BRDF loop's loss, its streaming backward pass, the normal step and Adam
(inverse_img_w_mi.py:371-432; include/matpbr.h `matpbr_brdf_loss_stats`, `matpbr_brdf_loss_dpred`, `matpbr_shade_bwd_jac`,
`matpbr_brdf_loss_bwd_jac`, `matpbr_brdf_normal_step`), in torch and nothing else: no project kernel, no renderer.

Every helper takes the fp32 tensors the kernels take and evaluates in `dtype` on `device` (default: double on the CPU, the reference of
tests/test_gpu_brdf_grad.py; with `dtype=torch.float32` the same closed form is the fp32 composition that test measures beside a kernel).
tests/test_brdf_fp64_host.py holds the double forms to torch autograd on `loss.brdf_loss` at 1e-10.

Layout: images and albedo [B,H,W,3], roughness / metallic [B,H,W,1], `maps` / `anchors` dicts with keys "a", "r", "m" (raw optimiser
parameters and the regulariser anchors), `jac` the nine planes [9,B,H,W] of matpbr_shade_fwd_ex (P rgb, S0 - S1 rgb, d out / d r rgb).
Per-image scalars are [B] tensors.  The roughness clamp's lower bound is the fp32 number nearest 0.07, the value torch.clamp compares fp32
maps with; `scale_delta` is rounded to fp32 likewise (both are fp32 arguments of the kernels)."""
import numpy as np
import torch

F64 = torch.float64
EPS = 1e-8                                   # loss._EPS: x^(1/2.2) has no gradient at or below it
LO_R = float(np.float32(0.07))
LIMS = {"a": (0.0, 1.0), "r": (LO_R, 1.0), "m": (0.0, 1.0)}
KEYS = ("a", "r", "m")
NORM_EPS = 1e-12                             # NF.normalize's eps

SHAPES = [(1, 1, 1), (1, 5, 7), (1, 16, 16), (1, 1, 257), (3, 33, 37), (2, 50, 70)]
PARTS = ["", "a", "r", "m", "rm", "am", "arm"]
STATS_PARTS = PARTS + ["n", "rn"]


def maps_in(part):
    """The material maps whose regulariser counts (include/matpbr.h: no material bit = all three; with 'n' exactly the ones named)."""
    named = [k for k in KEYS if k in part]
    return named if ("n" in part or named) else list(KEYS)


def _c(t, dtype, device):
    return t.detach().to(device=device, dtype=dtype)


def _mean(x):
    return x.reshape(x.shape[0], -1).mean(dim=1)


def _b(s, like):
    return s.reshape(-1, *([1] * (like.ndim - 1)))


def clamped(maps, dtype=F64, device="cpu"):
    return {k: _c(maps[k], dtype, device).clamp(*LIMS[k]) for k in KEYS if k in maps}


def stats64(pred, gt, maps, anchors, part, scale_delta, gt_srgb=None, dtype=F64, device="cpu"):
    """ratio, mse, l1, sr, la, lr, lm, loss per image ([B]) and the tone-mapped render `xs`, the target `gs` and `d = xs - gs`."""
    pred, gt = _c(pred, dtype, device), _c(gt, dtype, device)
    sd = float(np.float32(scale_delta))
    ratio = _mean(gt) / _mean(pred)
    xs = (pred * _b(ratio, pred)).clamp_min(EPS) ** (1.0 / 2.2)
    gs = gt ** (1.0 / 2.2) if gt_srgb is None else _c(gt_srgb, dtype, device)
    d = xs - gs
    mse, l1 = _mean(d * d), _mean(d.abs())
    sr = l1 / mse
    live, c = maps_in(part), clamped(maps, dtype, device)
    reg = {k: (_mean((c[k] - _c(anchors[k], dtype, device)).abs()) if k in live else torch.zeros_like(mse)) for k in KEYS}
    loss = 3.0 * sr * mse + l1 + sd * (reg["a"] + reg["r"] + reg["m"])
    return dict(ratio=ratio, mse=mse, l1=l1, sr=sr, la=reg["a"], lr=reg["r"], lm=reg["m"], loss=loss, xs=xs, gs=gs, d=d)


SLOTS = ("ratio", "mse", "l1", "sr", "la", "lr", "lm", "loss")     # slots 0..7 of a statistics row


def dpred64(pred, gt_srgb, ratio, sr, dtype=F64, device="cpu"):
    """d loss / d pred of 3 sr mse + l1 on xs = max(pred ratio, eps)^(1/2.2), ratio and sr constants."""
    pred, gs = _c(pred, dtype, device), _c(gt_srgb, dtype, device)
    ratio, sr = _b(_c(ratio, dtype, device), pred), _b(_c(sr, dtype, device), pred)
    x = pred * ratio
    xc = x.clamp_min(EPS)
    xs = xc ** (1.0 / 2.2)
    d = xs - gs
    n3 = pred[0].numel()
    return ratio * (x > EPS).to(dtype) * xs / (2.2 * xc) * (6.0 * sr * d + torch.sign(d)) / n3


def planes(jac, dtype=F64, device="cpu"):
    """[9,B,H,W] -> P, SD, JR as [B,H,W,3]."""
    j = _c(jac, dtype, device)
    return tuple(j[3 * k:3 * k + 3].permute(1, 2, 3, 0) for k in range(3))


def jac_grads64(a, r, m, P, SD, JR, go, dtype=F64, device="cpu"):
    """The material gradients of out_c = a_c (1-m) P_c + (m a_c + 0.04 (1-m)) SD_c + (terms in r with d out_c / d r = JR_c)."""
    a, m, P, SD, JR, go = (_c(t, dtype, device) for t in (a, m, P, SD, JR, go))
    d_a = go * (m * SD + (1.0 - m) * P)
    d_m = (go * ((a - 0.04) * SD - a * P)).sum(dim=-1, keepdim=True)
    d_r = (go * JR).sum(dim=-1, keepdim=True)
    return {"a": d_a, "r": d_r, "m": d_m}


def reg_and_gate64(maps, anchors, g, part, scale_delta, keys=KEYS, dtype=F64, device="cpu"):
    """g (w.r.t. the clamped maps) + scale_delta sign(clamp(p) - p0) / n for the maps of the part, through torch.clamp's backward:
    the gradient passes where lo <= raw <= hi, bounds included."""
    sd, live, out = float(np.float32(scale_delta)), maps_in(part), {}
    for k in keys:
        raw, lo, hi = _c(maps[k], dtype, device), *LIMS[k]
        gk = _c(g[k], dtype, device)
        if k in live:
            gk = gk + sd * torch.sign(raw.clamp(lo, hi) - _c(anchors[k], dtype, device)) / raw[0].numel()
        out[k] = torch.where((raw >= lo) & (raw <= hi), gk, torch.zeros_like(gk))
    return out


def fused_grads64(maps, anchors, pred, gt_srgb, ratio, sr, jac, part, scale_delta, dtype=F64, device="cpu"):
    """What matpbr_brdf_loss_bwd_jac writes into d_a, d_r, d_m (gradients with respect to the RAW maps)."""
    c = clamped(maps, dtype, device)
    go = dpred64(pred, gt_srgb, ratio, sr, dtype, device)
    P, SD, JR = planes(jac, dtype, device)
    g = jac_grads64(c["a"], c["r"], c["m"], P, SD, JR, go, dtype, device)
    return reg_and_gate64(maps, anchors, g, part, scale_delta, dtype=dtype, device=device)


def normalize64(v, dtype=F64, device="cpu"):
    v = _c(v, dtype, device)
    ln = v.norm(dim=-1, keepdim=True)
    return v / ln.clamp_min(NORM_EPS), ln


def normal_step_grads64(maps, anchors, d, pn, n0, part, scale_delta, dtype=F64, device="cpu"):
    """The gradients matpbr_brdf_normal_step hands to Adam: the material maps of the part as in `reg_and_gate64` from the given d["a"],
    d["r"], d["m"]; the normal g = d["n"] + scale_delta sign(n_hat - n0) / (3 H W) through NF.normalize's backward,
    (g - n_hat (n_hat . g)) / |v| where |v| > 1e-12 and g / 1e-12 below."""
    live = [k for k in KEYS if k in part]
    out = reg_and_gate64(maps, anchors, d, part if live else "n", scale_delta, keys=live, dtype=dtype, device=device)
    if "n" in part:
        nh, ln = normalize64(pn, dtype, device)
        g = _c(d["n"], dtype, device) + float(np.float32(scale_delta)) * torch.sign(nh - _c(n0, dtype, device)) / nh[0].numel()
        den = ln.clamp_min(NORM_EPS)
        out["n"] = torch.where(ln > NORM_EPS, (g - nh * (nh * g).sum(dim=-1, keepdim=True)) / den, g / den)
    return out


def adam64(p, g, m, v, lr, t, b1=0.9, b2=0.999, eps=1e-8, dtype=F64, device="cpu"):
    """torch.optim.Adam's update (no weight decay, no amsgrad) of step t (1-based): returns the new (p, m, v)."""
    p, g, m, v = (_c(x, dtype, device) for x in (p, g, m, v))
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    denom = v.sqrt() / (1.0 - b2 ** t) ** 0.5 + eps
    return p - (lr / (1.0 - b1 ** t)) * m / denom, m, v


# ------------------------------------------------------------------------------------------------------------------------------
# the inputs of tests/test_gpu_brdf_grad.py (fp32, CPU, seeded by the shape): built here so that tests/test_brdf_fp64_host.py checks the
# conditions they are meant to meet without a GPU
# ------------------------------------------------------------------------------------------------------------------------------
def _spread(gen, shape):
    """Magnitudes 1e-3 ... 10 (log-uniform), random signs."""
    return 10.0 ** (torch.rand(shape, generator=gen) * 4.0 - 3.0) * (torch.randint(0, 2, shape, generator=gen) * 2.0 - 1.0)


def _raw_map(gen, shape, lo, hi):
    """A raw parameter map and its anchor.  Twenty classes of elements in a seeded permutation (every class occurs from 20 elements on):
    below / above the clamp range, exactly on 0, 1 and 0.07, clamp(p) == p0 inside the range and on either bound from outside, and
    the rest inside the range at least 2e-3 from the anchor."""
    n = int(np.prod(shape))
    p0 = lo + 0.05 + (hi - lo - 0.1) * torch.rand(n, generator=gen)
    raw = lo + (hi - lo) * torch.rand(n, generator=gen)
    near = (raw - p0).abs() < 2e-3
    raw = torch.where(near, p0 + 2e-3 * torch.where(raw >= p0, 1.0, -1.0), raw)
    cls = torch.randperm(n, generator=gen) % 20
    u = 0.01 + 0.29 * torch.rand(n, generator=gen)
    raw = torch.where(cls == 0, lo - u, raw)
    raw = torch.where(cls == 1, hi + u, raw)
    raw = torch.where(cls == 2, torch.zeros(n), raw)
    raw = torch.where(cls == 3, torch.ones(n), raw)
    raw = torch.where(cls == 4, torch.full((n,), 0.07), raw)
    p0 = torch.where((cls == 4) & ((p0 - 0.07).abs() < 2e-3), p0 + 0.01, p0)
    raw = torch.where(cls == 5, p0, raw)                                              # sign 0, gate open
    p0 = torch.where(cls == 6, torch.full((n,), float(lo)), p0)                        # sign 0 on the lower bound, gate closed
    raw = torch.where(cls == 6, lo - u, raw)
    p0 = torch.where(cls == 7, torch.full((n,), float(hi)), p0)                        # sign 0 on the upper bound, gate closed
    raw = torch.where(cls == 7, hi + u, raw)
    return raw.reshape(shape).float().contiguous(), p0.reshape(shape).float().contiguous()


def make_inputs(B, H, W):
    """Everything the kernel tests feed, as fp32 CPU tensors (see the module docstring for the layout)."""
    gen = torch.Generator().manual_seed(20251018 + 1000003 * B + 1009 * H + W)
    s3, s1 = (B, H, W, 3), (B, H, W, 1)
    gt = 0.05 + 0.8 * torch.rand(s3, generator=gen)
    f = 0.55 + 0.3 * torch.rand(s3, generator=gen) + 0.6 * torch.randint(0, 2, s3, generator=gen)
    pred = (gt * f).float().contiguous()
    n3 = H * W * 3
    pred_z = pred.clone()                      # a handful of exact zeros per image (none in an image of fewer than 24 values)
    zeros = torch.zeros(s3, dtype=torch.bool)
    for b in range(B):
        idx = torch.randperm(n3, generator=gen)[: min(5, n3 // 24)]
        zeros[b].view(-1)[idx] = True
    pred_z[zeros] = 0.0
    maps, anchors = {}, {}
    for k, shp in (("a", s3), ("r", s1), ("m", s1)):
        maps[k], anchors[k] = _raw_map(gen, shp, float(np.float32(LIMS[k][0])), 1.0)
    jac = _spread(gen, (9, B, H, W)).float().contiguous()
    go = (_spread(gen, s3) / n3).float().contiguous()
    # the normal step's own inputs: upstream gradients of the size of d loss / d pred, non-unit normals of length 0.3 ... 3, anchors at
    # least 1e-3 from the unit normal in every component; per image one axis-aligned vector of a power-of-two length whose unit normal
    # is exact in any arithmetic (n_hat == n0 in two components), and one all-zero vector
    d = {k: (_spread(gen, shp) / n3).float().contiguous() for k, shp in (("a", s3), ("r", s1), ("m", s1), ("n", s3))}
    dirs = torch.nn.functional.normalize(torch.randn(s3, generator=gen, dtype=F64), dim=-1)
    pn = dirs * (0.3 + 2.7 * torch.rand(s1, generator=gen, dtype=F64))
    n0 = torch.nn.functional.normalize(dirs + 0.2 * torch.randn(s3, generator=gen, dtype=F64), dim=-1)
    pn, n0 = pn.float(), n0.float()
    nh = torch.nn.functional.normalize(pn.double(), dim=-1)
    close = (nh - n0.double()).abs() < 2e-3
    n0 = torch.where(close, (nh + 4e-3).float(), n0)
    exact_pix, zero_pix = [], []
    P = H * W
    for b in range(B):
        if P >= 3:
            e, z = int(torch.randint(0, P, (1,), generator=gen)), int(torch.randint(0, P, (1,), generator=gen))
            z = z if z != e else (e + 1) % P
            pn[b].view(P, 3)[e] = torch.tensor([0.0, -2.0, 0.0])
            n0[b].view(P, 3)[e] = torch.tensor([0.0, -1.0, 0.25])
            pn[b].view(P, 3)[z] = 0.0
            exact_pix.append(e)
            zero_pix.append(z)
    return dict(B=B, H=H, W=W, gt=gt.float().contiguous(), gt_srgb=(gt.float() ** (1.0 / 2.2)).contiguous(), pred=pred, pred_z=pred_z, zeros=zeros,
                maps=maps, anchors=anchors, jac=jac, go=go, d=d, pn=pn.contiguous(), n0=n0.contiguous(), exact_pix=exact_pix, zero_pix=zero_pix)


class _RenderFromPlanes(torch.autograd.Function):
    """A render node for the torch composition: its value is the given image, its backward the closed forms of the jac planes in the
    dtype of the incoming gradient (what render_w_brdf's node does with the renderer's planes)."""

    @staticmethod
    def forward(ctx, a, r, m, pred, jac):
        ctx.save_for_backward(a, m, jac)
        return pred.clone()

    @staticmethod
    def backward(ctx, go):
        a, m, jac = ctx.saved_tensors
        g = jac_grads64(a, None, m, *planes(jac, go.dtype, go.device), go, go.dtype, go.device)
        return g["a"], g["r"], g["m"], None, None


def torch_composition(loss_module, maps, anchors, pred, gt, gt_srgb, jac, part, scale_delta, dtype, device="cpu"):
    """`loss.brdf_loss` (the caller sets `loss.FUSED = False`) around clamps and the render node above, differentiated by autograd in
    `dtype`: the gradients of the raw maps, d loss / d pred, and loss_mse, ratio [B] and the summed loss as brdf_loss returns them."""
    names = {"a": "albedo", "r": "roughness", "m": "metallic"}
    raw = {k: _c(maps[k], dtype, device).requires_grad_() for k in KEYS}
    c = {k: raw[k].clamp(*LIMS[k]) for k in KEYS}
    out = _RenderFromPlanes.apply(c["a"], c["r"], c["m"], _c(pred, dtype, device), _c(jac, dtype, device))
    out.retain_grad()
    live = maps_in(part)
    total, mse, xs, ratio = loss_module.brdf_loss(out, _c(gt, dtype, device), {names[k]: c[k] for k in live},
                                                  {names[k]: _c(anchors[k], dtype, device) for k in live}, float(np.float32(scale_delta)),
                                                  gt_srgb=_c(gt_srgb, dtype, device))
    total.backward()
    return {k: raw[k].grad for k in KEYS}, out.grad, mse.detach().reshape(-1), ratio.detach().reshape(-1), total.detach(), xs.detach()


def sign_exclusions(pred, gt, gt_srgb, maps, anchors):
    """Section 5.2's condition: the elements whose sign(xs - gt_srgb) may differ between fp32 and fp64 are those with |d| < 1e-5 in the
    fp64 reference.  Returns (that mask, the smallest |d|, the number of fp32 / fp64 sign disagreements of the CPU composition)."""
    s64 = stats64(pred, gt, maps, anchors, "arm", 0.1, gt_srgb)
    s32 = stats64(pred, gt, maps, anchors, "arm", 0.1, gt_srgb, dtype=torch.float32)
    flips = int((torch.sign(s64["d"]) != torch.sign(s32["d"].double())).sum())
    return s64["d"].abs() < 1e-5, float(s64["d"].abs().min()), flips
