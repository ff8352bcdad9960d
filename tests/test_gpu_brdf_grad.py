"""The `--model_name none` BRDF loop's loss and streaming backward kernels against fp64, one entry point at a time.

Every other test of this loop looks at parameters after a few Adam steps, and Adam's first steps are +-lr whatever the gradient's size: a
wrong constant in `jac_bwd_kernel<FUSED>`, a regulariser over the wrong element count or a missing `ratio` moves nothing those tests see.
Here the statistics, d loss / d pred, the material gradients of `matpbr_shade_bwd_jac` and `matpbr_brdf_loss_bwd_jac` (fp32 and half
planes), the exact phase's `g`, `m`, `p` over two steps and `matpbr_brdf_normal_step`'s applied gradients are read directly and compared
with the plain fp64 helpers of tests/brdf_fp64.py (held to autograd by tests/test_brdf_fp64_host.py), on random planes: no renderer in (a)-(d), (f).

Bound (section 5.1's rule): every comparison is max |got - ref64| / max |ref64| of one tensor; beside the kernel's error the test measures
e_torch32, the fp32 torch composition of the same operation on the GPU (`loss.brdf_loss` with FUSED = False plus autograd; the closed forms
in fp32 for the plain backward and the normal step), and asserts e_kernel <= max(4 e_torch32, FLOOR).  FLOOR = 2.6e-6 is four times the
worst error of that composition on a CPU over this file's inputs (6.4e-7: the fused d_r; tests/test_brdf_fp64_host.py prints the figures).
Parameters after Adam are compared as |p - p64| / lr under the same rule.  Gates, regulariser signs, snapshots of clamped maps, NaN guards
and untouched outputs are exact.  No element is left out of a comparison: the inputs keep |xs - gt_srgb| above 1e-2 (the host test
asserts it), and the test fails if more than 0.1 % of a tensor would have to be."""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import brdf_fp64 as bf  # noqa: E402
from test_gpu_env_grad import _Tally as _EnvTally, _report  # noqa: E402

FLOOR = 2.6e-6
SD = 0.1
LR = 3e-4
NAN = float("nan")
GUARD = 256
B1, B2 = float(np.float32(0.9)), float(np.float32(0.999))    # the kernels' betas are fp32 arguments: torch.optim.Adam with these betas
ONE_MINUS_B1 = float(np.float32(1.0) - np.float32(0.9))      # (1.0f - b1) of the kernels' Adam
_IDS = ["x".join(map(str, s)) for s in bf.SHAPES]
_NAME = {"a": "albedo", "r": "roughness", "m": "metallic", "n": "normal"}


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.manual_seed(20251018)
    return torch.device("cuda:0")


def _rel(got, ref):
    return (got.detach().double().cpu() - ref).abs().max().item() / (ref.abs().max().item() + 1e-300)


class _Tally(_EnvTally):
    """tests/test_gpu_env_grad.py's tally (measure, print, report, assert at the end) on CPU references, with this file's floor."""

    def bounded(self, what, got, ref64, t32, floor=FLOOR, scale=None):
        got, t32, ref64 = got.detach().double().cpu(), t32.detach().double().cpu().reshape(ref64.shape), ref64.detach().cpu()
        assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
        finite = bool(torch.isfinite(got).all())
        den = scale if scale is not None else ref64.abs().max().item() + 1e-300
        e_k = (got - ref64).abs().max().item() / den if finite else float("inf")
        e_t = (t32 - ref64).abs().max().item() / den
        bound = max(4.0 * e_t, floor)
        print(f"{what}: e_kernel {e_k:.3e}  e_torch32 {e_t:.3e}  bound {bound:.3e}")
        _report(what, e_k, bound)
        _report(what + " [fp32 torch composition]", e_t, float("inf"))
        if not finite:
            self.bad.append(f"{what}: non-finite values")
        elif not e_k <= bound:
            self.bad.append(f"{what}: e_kernel {e_k:.3e} > max(4 x e_torch32 {e_t:.3e}, {floor:.1e})")


def _lib():
    from materialist_amd import _lib as L

    return L.load()


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class _Out:
    """An output buffer that starts as NaN, with a NaN guard row behind it."""

    def __init__(self, dev, *shape, dtype=torch.float32):
        n = int(np.prod(shape))
        self.flat = torch.full((n + GUARD,), NAN, dtype=torch.float32, device=dev)
        self.t = self.flat[:n].view(*shape)
        self.dtype = dtype

    def guard_ok(self):
        return bool(torch.isnan(self.flat[self.t.numel():]).all())

    def all_nan(self):
        return bool(torch.isnan(self.flat).all())


def _bits_equal(x, y):
    return x.shape == y.shape and bool((x.contiguous().view(torch.int32) == y.contiguous().view(torch.int32)).all())


@pytest.fixture(scope="module")
def inputs():
    return {s: bf.make_inputs(*s) for s in bf.SHAPES}


@pytest.fixture()
def torch_loss():
    from materialist_amd import loss

    keep, loss.FUSED = loss.FUSED, False
    yield loss
    loss.FUSED = keep


def _to(dev, inp):
    g = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}
    for k in ("maps", "anchors", "d"):
        g[k] = {q: v.to(dev) for q, v in inp[k].items()}
    return g


def _row(dev, B, s64=None, improved=1.0, best=None):
    """Statistics rows [B,16]: NaN except `stopped` and `iterations` (0) and what is given -- the fp64 statistics rounded to fp32."""
    st = torch.full((B, 16), NAN, dtype=torch.float32)
    st[:, 13], st[:, 14] = 0.0, 0.0
    if s64 is not None:
        for i, k in enumerate(bf.SLOTS):
            st[:, i] = s64[k].float()
        st[:, 8] = improved
    if best is not None:
        st[:, 9] = best
    return st.to(dev)


def _excluded(s64, per_pixel=False, builder=True):
    """Section 5.2's sign condition: elements with |xs - gt_srgb| < 1e-5 in the fp64 reference are left out of the element-wise gradient
    comparisons, at most 0.1 % of a tensor; none at all of the builder's inputs (tests/test_brdf_fp64_host.py)."""
    mask = s64["d"].abs() < 1e-5
    assert int(mask.sum()) <= 1e-3 * mask.numel()
    assert not builder or int(mask.sum()) == 0
    return mask.any(dim=-1, keepdim=True) if per_pixel else mask


def _stats_call(g, dev, pred, part, st, ws, sel=None):
    from materialist_amd import ops

    B, H, W = g["B"], g["H"], g["W"]
    pick = (lambda t: t) if sel is None else (lambda t: t[sel:sel + 1].contiguous())
    Bc = B if sel is None else 1
    with torch.cuda.device(dev):
        code = _lib().matpbr_brdf_loss_stats_es(_P(pick(pred)), _P(pick(g["gt"])), _P(pick(g["gt_srgb"])), _P(pick(g["maps"]["a"])), _P(pick(g["maps"]["r"])),
                                                _P(pick(g["maps"]["m"])), _P(pick(g["anchors"]["a"])), _P(pick(g["anchors"]["r"])), _P(pick(g["anchors"]["m"])),
                                                SD, _P(st), _P(ws), ws.numel() * 4, H, W, Bc, ops.part_mask(part), 0, 0.0, None, 0, _stream(dev))
    assert code == 0, code


# ------------------------------------------------------------------------------------------------------------------------------
# a. matpbr_brdf_loss_stats_es
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", bf.SHAPES, ids=_IDS)
def test_loss_statistics_match_fp64(shape, inputs, torch_loss):
    """Slots ratio, mse, l1, sr, la, lr, lm, loss for every part; la / lr / lm exactly 0 outside the part; SaveBest's strict `<` against a
    best_mse planted 1e-4 above and below the fp64 mse; the other slots untouched; a batch row = its image alone, bit for bit."""
    dev = _cuda()
    inp = inputs[shape]
    g = _to(dev, inp)
    B = shape[0]
    lib = _lib()
    ws_n = int(lib.matpbr_brdf_loss_workspace_bytes(B)) // 4
    T = _Tally()
    for pred_key in ("pred", "pred_z"):
        for part in bf.STATS_PARTS:
            if pred_key == "pred_z" and part != "arm":
                continue
            s64 = bf.stats64(inp[pred_key], inp["gt"], inp["maps"], inp["anchors"], part, SD, inp["gt_srgb"])
            s32 = bf.stats64(g[pred_key], g["gt"], g["maps"], g["anchors"], part, SD, g["gt_srgb"], dtype=torch.float32, device=dev)
            live = bf.maps_in(part)
            with torch.no_grad():      # ratio, mse and loss of the torch composition, image by image (brdf_loss returns the batch's summed loss)
                c = bf.clamped(g["maps"], torch.float32, dev)
                rows = [torch_loss.brdf_loss(g[pred_key][b:b + 1], g["gt"][b:b + 1], {_NAME[k]: c[k][b:b + 1] for k in live},
                                             {_NAME[k]: g["anchors"][k][b:b + 1] for k in live}, float(np.float32(SD)), gt_srgb=g["gt_srgb"][b:b + 1]) for b in range(B)]
            s32.update(loss=torch.stack([r[0] for r in rows]), mse=torch.cat([r[1].reshape(-1) for r in rows]), ratio=torch.cat([r[3].reshape(-1) for r in rows]))
            for side, factor in (("above", 1.0 + 1e-4), ("below", 1.0 - 1e-4)):
                if side == "below" and part != "arm":
                    continue
                best = (s64["mse"] * factor).float()
                st, ws = _row(dev, B, best=best), _Out(dev, ws_n)
                stg = _Out(dev, B, 16)
                stg.t.copy_(st)
                _stats_call(g, dev, g[pred_key], part, stg.t, ws.t)
                torch.cuda.synchronize()
                got = stg.t.cpu()
                tag = f"stats {pred_key} part '{part}' best {side}"
                T.exact(f"{tag}: guard rows", stg.guard_ok() and ws.guard_ok())
                T.exact(f"{tag}: slots 10, 11, 12, 15 stay NaN, stopped stays 0", bool(torch.isnan(got[:, [10, 11, 12, 15]]).all()) and bool((got[:, 13] == 0).all()))
                T.exact(f"{tag}: iterations counted", bool((got[:, 14] == 1).all()))
                if side == "above":
                    for i, k in enumerate(bf.SLOTS):
                        if k in ("la", "lr", "lm") and k[1] not in live:
                            T.exact(f"{tag}: {k} is exactly 0 outside the part", bool((got[:, i] == 0).all()) and not bool(torch.signbit(got[:, i]).any()))
                        else:
                            T.bounded(f"{tag} {k}", got[:, i], s64[k], s32[k])
                    T.exact(f"{tag}: improved, best = mse", bool((got[:, 8] == 1).all()) and _bits_equal(got[:, 9], got[:, 1]))
                    if B > 1 and part == "arm":
                        for b in range(B):
                            one = _Out(dev, 1, 16)
                            one.t.copy_(st[b:b + 1])
                            _stats_call(g, dev, g[pred_key], part, one.t, _Out(dev, int(lib.matpbr_brdf_loss_workspace_bytes(1)) // 4).t, sel=b)
                            torch.cuda.synchronize()
                            T.exact(f"{tag}: image {b} alone = its batch row, bit for bit", _bits_equal(one.t[0, :10].cpu(), got[b, :10]))
                else:
                    T.exact(f"{tag}: not improved, best kept", bool((got[:, 8] == 0).all()) and _bits_equal(got[:, 9], best))
    T.done()


# ------------------------------------------------------------------------------------------------------------------------------
# b. matpbr_brdf_loss_dpred
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", bf.SHAPES, ids=_IDS)
def test_dpred_matches_fp64(shape, inputs, torch_loss):
    """Every element of d loss / d pred from a statistics row that holds the fp64 ratio and sr rounded to fp32; exact zeros where the render
    is zero; an image whose row says `stopped earlier` keeps its NaN."""
    from materialist_amd import ops

    dev = _cuda()
    inp = inputs[shape]
    g = _to(dev, inp)
    B = shape[0]
    T = _Tally()
    s64 = bf.stats64(inp["pred_z"], inp["gt"], inp["maps"], inp["anchors"], "arm", SD, inp["gt_srgb"])
    ex = _excluded(s64)
    st = _row(dev, B, s64)
    ref = bf.dpred64(inp["pred_z"], inp["gt_srgb"], st[:, 0].cpu(), st[:, 3].cpu())
    _, t32, _, _, _, _ = bf.torch_composition(torch_loss, g["maps"], g["anchors"], g["pred_z"], g["gt"], g["gt_srgb"], g["jac"], "arm", SD, torch.float32, dev)
    out = _Out(dev, *inp["pred"].shape)
    ops.brdf_loss_dpred(g["pred_z"], g["gt_srgb"], st, out.t)
    torch.cuda.synchronize()
    got = out.t.clone()
    T.bounded("d_pred", torch.where(ex.to(dev), ref.float().to(dev), got), ref, t32)
    T.exact("d_pred: guard row", out.guard_ok())
    T.exact("d_pred: exactly 0 where the render is 0", bool((got[g["zeros"]] == 0).all()) and bool((ref[inp["zeros"]] == 0).all()))
    T.exact("d_pred: non-zero elsewhere", bool((got[~g["zeros"]] != 0).all()))
    # the last image stopped in an earlier iteration: its gradient is not written
    st2 = st.clone()
    st2[B - 1, 13] = 2.0
    out2 = _Out(dev, *inp["pred"].shape)
    ops.brdf_loss_dpred(g["pred_z"], g["gt_srgb"], st2, out2.t)
    torch.cuda.synchronize()
    T.exact("d_pred: a stopped image keeps its NaN", bool(torch.isnan(out2.t[B - 1]).all()) and out2.guard_ok())
    T.exact("d_pred: the running images are written as before", B == 1 or _bits_equal(out2.t[:B - 1], got[:B - 1]))
    st2[B - 1, 13] = 1.0      # EarlyStopping fired in THIS iteration: it still runs to its end
    out3 = _Out(dev, *inp["pred"].shape)
    ops.brdf_loss_dpred(g["pred_z"], g["gt_srgb"], st2, out3.t)
    torch.cuda.synchronize()
    T.exact("d_pred: the firing iteration is still written", _bits_equal(out3.t, got))
    T.done()


# ------------------------------------------------------------------------------------------------------------------------------
# c. matpbr_shade_bwd_jac (jac_bwd_kernel<false>)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", bf.SHAPES, ids=_IDS)
def test_shade_bwd_jac_matches_fp64(shape, inputs):
    dev = _cuda()
    inp = inputs[shape]
    g = _to(dev, inp)
    B, H, W = shape
    T = _Tally()
    c32 = bf.clamped(g["maps"], torch.float32, dev)
    c32 = {k: v.contiguous() for k, v in c32.items()}
    ref = bf.jac_grads64(c32["a"].cpu(), None, c32["m"].cpu(), *bf.planes(inp["jac"]), inp["go"])
    t32 = bf.jac_grads64(c32["a"], None, c32["m"], *bf.planes(g["jac"], torch.float32, dev), g["go"], dtype=torch.float32, device=dev)
    outs = {"a": _Out(dev, B, H, W, 3), "r": _Out(dev, B, H, W, 1), "m": _Out(dev, B, H, W, 1)}
    with torch.cuda.device(dev):
        code = _lib().matpbr_shade_bwd_jac(_P(c32["a"]), _P(c32["r"]), _P(c32["m"]), _P(g["jac"]), _P(g["go"]), _P(outs["a"].t), _P(outs["r"].t), _P(outs["m"].t),
                                           H, W, B, _stream(dev))
    assert code == 0
    torch.cuda.synchronize()
    for k in bf.KEYS:
        T.bounded(f"shade_bwd_jac d_{k}", outs[k].t, ref[k], t32[k])
        T.exact(f"shade_bwd_jac d_{k}: guard row", outs[k].guard_ok())
    T.done()


# ------------------------------------------------------------------------------------------------------------------------------
# d. matpbr_brdf_loss_bwd_jac, fp32 planes and MATPBR_FLAG_JAC16
# ------------------------------------------------------------------------------------------------------------------------------
def _pack_jac16(jac):
    """The five planes of 32-bit words matpbr_brdf_loss_bwd_jac(MATPBR_FLAG_JAC16) reads -- half2 (P_c, SD_c) x rgb, (JR_0, JR_1), (JR_2, 0),
    the first half in the low 16 bits -- and the nine planes as the kernel sees them (rounded to half)."""
    h = jac.half()
    bits = h.view(torch.int16).to(torch.int64) & 0xFFFF

    def pair(lo, hi):
        w = lo | (hi << 16)
        return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)

    zero = torch.zeros_like(bits[0])
    words = torch.stack([pair(bits[0], bits[3]), pair(bits[1], bits[4]), pair(bits[2], bits[5]), pair(bits[6], bits[7]), pair(bits[8], zero)])
    return words.contiguous(), h.float().contiguous()


@pytest.mark.parametrize("jac16", [False, True], ids=["planes32", "planes16"])
@pytest.mark.parametrize("shape", bf.SHAPES, ids=_IDS)
def test_loss_bwd_jac_matches_fp64(shape, jac16, inputs, torch_loss):
    """d_a, d_r, d_m of every part element by element, from a statistics row that holds stats64's values (an error of the statistics kernels
    cannot cancel here); the clamp gates exactly (0.0 outside the range, non-zero on the bounds); SaveBest's snapshots both ways."""
    from materialist_amd import ops

    dev = _cuda()
    inp = inputs[shape]
    g = _to(dev, inp)
    B, H, W = shape
    T = _Tally()
    if jac16:
        words, jac_seen = _pack_jac16(g["jac"])
        jac_arg = torch.full((9, B, H, W), NAN, dtype=torch.float32, device=dev)      # room of matpbr_plane9_bytes(), the words in its first five planes
        jac_arg.view(torch.int32)[:5] = words
    else:
        jac_arg = jac_seen = g["jac"]
    c32 = bf.clamped(g["maps"], torch.float32, dev)
    for part in bf.PARTS:
        s64 = bf.stats64(inp["pred_z"], inp["gt"], inp["maps"], inp["anchors"], part, SD, inp["gt_srgb"])
        ex = _excluded(s64, per_pixel=True)
        st = _row(dev, B, s64, improved=1.0, best=s64["mse"].float())
        ref = bf.fused_grads64(inp["maps"], inp["anchors"], inp["pred_z"], inp["gt_srgb"], st[:, 0].cpu(), st[:, 3].cpu(), jac_seen.cpu(), part, SD)
        xs_ref = (inp["pred_z"].double() * st[:, 0].cpu().double().reshape(B, 1, 1, 1)).clamp_min(bf.EPS) ** (1.0 / 2.2)
        t32, _, _, _, _, xs32 = bf.torch_composition(torch_loss, g["maps"], g["anchors"], g["pred_z"], g["gt"], g["gt_srgb"], jac_seen, part, SD, torch.float32, dev)
        outs = {k: _Out(dev, *inp["maps"][k].shape) for k in bf.KEYS}
        best = {k: _Out(dev, *inp["maps"][k].shape) for k in bf.KEYS}
        best_img = _Out(dev, B, H, W, 3)
        ops.brdf_loss_bwd_jac(g["maps"]["a"], g["maps"]["r"], g["maps"]["m"], jac_arg, g["pred_z"], g["gt_srgb"], st, g["anchors"]["a"], g["anchors"]["r"],
                              g["anchors"]["m"], SD, outs["a"].t, outs["r"].t, outs["m"].t, best["a"].t, best["r"].t, best["m"].t, best_img.t,
                              optimize_part=part, jac16=jac16)
        torch.cuda.synchronize()
        tag = f"loss_bwd_jac part '{part}'"
        for k in bf.KEYS:
            got, raw, (lo, hi) = outs[k].t.clone(), g["maps"][k], bf.LIMS[k]
            T.bounded(f"{tag} d_{k}", torch.where(ex.to(dev).expand_as(got), ref[k].float().to(dev), got), ref[k], t32[k])
            outside, on_bound = (raw < lo) | (raw > hi), (raw == float(np.float32(lo))) | (raw == hi)
            dark = g["zeros"] if k == "a" else g["zeros"].all(dim=-1, keepdim=True)     # the render's planted zeros: no data term there
            T.exact(f"{tag} d_{k}: exactly 0 outside the clamp range", bool((got[outside] == 0).all()) and bool((ref[k][outside.cpu()] == 0).all()))
            T.exact(f"{tag} d_{k}: non-zero on the bounds and inside", bool((got[~outside & ~dark] != 0).all()) and (raw.numel() < 40 or bool(on_bound.any())))
            T.exact(f"{tag} d_{k}: guard rows", outs[k].guard_ok() and best[k].guard_ok())
            T.exact(f"{tag} best_{k} = the clamped map", _bits_equal(best[k].t, c32[k]))
        T.bounded(f"{tag} best_img", best_img.t, xs_ref, xs32)
        T.exact(f"{tag} best_img: guard row", best_img.guard_ok())
        if part in ("arm", "r"):         # not improved: the same gradients, no snapshot
            st0 = st.clone()
            st0[:, 8] = 0.0
            outs0 = {k: _Out(dev, *inp["maps"][k].shape) for k in bf.KEYS}
            best0 = {k: _Out(dev, *inp["maps"][k].shape) for k in bf.KEYS}
            img0 = _Out(dev, B, H, W, 3)
            ops.brdf_loss_bwd_jac(g["maps"]["a"], g["maps"]["r"], g["maps"]["m"], jac_arg, g["pred_z"], g["gt_srgb"], st0, g["anchors"]["a"], g["anchors"]["r"],
                                  g["anchors"]["m"], SD, outs0["a"].t, outs0["r"].t, outs0["m"].t, best0["a"].t, best0["r"].t, best0["m"].t, img0.t,
                                  optimize_part=part, jac16=jac16)
            torch.cuda.synchronize()
            T.exact(f"{tag}: improved = 0 leaves the snapshots NaN", all(best0[k].all_nan() for k in bf.KEYS) and img0.all_nan())
            T.exact(f"{tag}: improved = 0 writes the same gradients", all(_bits_equal(outs0[k].t, outs[k].t) for k in bf.KEYS))
    T.done()


# ------------------------------------------------------------------------------------------------------------------------------
# e. the exact phase: FusedBrdfPhase(lazy=False, keep_grads=True), two steps
# ------------------------------------------------------------------------------------------------------------------------------
def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)


def _scene_inputs(dev, B, H, W, first_id):
    from materialist_amd import synthetic

    scs = [synthetic.make_scene(first_id + i, H, W) for i in range(B)]
    st = (lambda f: torch.stack([_t(f(s), dev) for s in scs])) if B > 1 else (lambda f: _t(f(scs[0]), dev))
    init = [st(lambda s: s.init_albedo), st(lambda s: s.init_roughness), st(lambda s: s.init_metallic)]
    init[1] = init[1] + 0.2 * (torch.rand(init[1].shape, device=dev) - 0.5)      # the start roughness / metallic are constants in make_scene
    init[2] = init[2] + 0.3 * torch.rand(init[2].shape, device=dev)
    for k, (below, above) in enumerate(((-0.2, 1.2), (0.01, 1.3), (-0.3, 1.1))):     # a few raw values outside the clamps, on either side
        flat = init[k].view(-1)
        flat[1::11] = below
        flat[5::13] = above
    true = [st(lambda s: s.albedo), st(lambda s: s.roughness), st(lambda s: s.metallic)]
    return st(lambda s: s.depth), st(lambda s: s.light), [x.contiguous() for x in init], true


def _stats32(torch_loss, dev, pred, gt, gt_srgb, maps, anchors, part):
    """The fp32 torch statistics on the GPU: stats64's expression in fp32, with ratio, mse and loss from loss.brdf_loss image by image."""
    s32 = bf.stats64(pred, gt, maps, anchors, part, SD, gt_srgb, dtype=torch.float32, device=dev)
    live, c = bf.maps_in(part), bf.clamped(maps, torch.float32, dev)
    with torch.no_grad():
        rows = [torch_loss.brdf_loss(pred[b:b + 1], gt[b:b + 1], {_NAME[k]: c[k][b:b + 1] for k in live}, {_NAME[k]: anchors[k][b:b + 1] for k in live},
                                     float(np.float32(SD)), gt_srgb=gt_srgb[b:b + 1]) for b in range(pred.shape[0])]
    s32.update(loss=torch.stack([r[0] for r in rows]), mse=torch.cat([r[1].reshape(-1) for r in rows]), ratio=torch.cat([r[3].reshape(-1) for r in rows]))
    return s32


@pytest.mark.parametrize("part", ["arm", "rm", "a"])
@pytest.mark.parametrize("size", [(1, 5, 7), (1, 33, 37), (2, 16, 16)], ids=["5x7", "33x37", "2x16x16"])
def test_exact_phase_gradients_and_adam_match_fp64(size, part, torch_loss):
    """After each of two steps: the statistics row against stats64 of the phase's own render; `g` against fused_grads64 on the planes of a
    render at the maps the step started from; `m`, `v`, `p` of the part's maps against adam64 carried over both steps (bias corrections and
    step count, with a second gradient that differs from the first), fed with the gradient the kernel wrote; the other maps bit-unchanged.
    Regression: in part 'a' the phase used to combine the first render's planes in later steps, and `g_r` of step 2 was the roughness gradient
    as of step 1's albedo (1.1e-3 ... 3.2e-3 of its maximum off); with `keep_grads` it now walks the samples in every step."""
    from materialist_amd import loop, ops, render

    dev = _cuda()
    B, H, W = size
    spp = 8
    depth, light, init, true = _scene_inputs(dev, B, H, W, 40)

    def make_scene():
        s = render.load_estimated_mesh(depth, use_mesh_normal=True)
        s._set("emitter.data", light)
        return s

    with torch.no_grad():
        gt = render.render_w_brdf(make_scene(), *true, None, spp)
    originals = {"albedo": (init[0] * 0.9).clamp(0.02, 0.98), "roughness": (init[1] * 0.9).clamp(0.1, 0.9), "metallic": (init[2] * 0.9 + 0.02).clamp(0.02, 0.9)}
    ph = loop.FusedBrdfPhase(make_scene(), gt, *init, optimize_part=part, spp=spp, lr=LR, lazy=False, keep_grads=True, originals=originals)
    shp = lambda t, c: t.reshape(B, H, W, c)
    anchors = {k: shp(ph.orig[_NAME[k]], 3 if k == "a" else 1) for k in bf.KEYS}
    gt4, gs4 = shp(ph.gt, 3), shp(ph.gt_srgb, 3)
    T = _Tally()
    m64 = {k: torch.zeros(anchors[k].shape, dtype=torch.float64) for k in part}
    v64 = {k: torch.zeros(anchors[k].shape, dtype=torch.float64) for k in part}
    m32 = {k: torch.zeros_like(anchors[k]) for k in part}
    v32 = {k: torch.zeros_like(anchors[k]) for k in part}
    g_first = None
    for t in (1, 2):
        start = {k: shp(ph.p[_NAME[k]], 3 if k == "a" else 1).clone() for k in bf.KEYS}
        ph.step()
        torch.cuda.synchronize()
        pred = shp(ph.pred, 3).clone()
        tag = f"phase {part} step {t}"
        # the statistics row
        cpu = lambda d: {k: v.cpu() for k, v in d.items()}
        s64 = bf.stats64(pred.cpu(), gt4.cpu(), cpu(start), cpu(anchors), part, SD, gs4.cpu())
        ex = _excluded(s64, per_pixel=True, builder=False)
        s32 = _stats32(torch_loss, dev, pred, gt4, gs4, start, anchors, part)
        row = ph.stats.cpu()
        for i, k in enumerate(bf.SLOTS):
            if k in ("la", "lr", "lm") and k[1] not in part:
                T.exact(f"{tag} stats {k}: exactly 0 outside the part", bool((row[:, i] == 0).all()))
            else:
                T.bounded(f"{tag} stats {k}", row[:, i], s64[k], s32[k])
        T.exact(f"{tag}: iterations counted", bool((row[:, 14] == t).all()))
        # the gradients, on the planes of a render at the step's start maps
        jac = ops.plane9(start["a"])
        again = ops.shade_fwd(start["a"], start["r"], start["m"], ph.n, ph.light, spp, ph.scene.fov, clamp_params=True, dcache=ph.dcache, jac=jac)
        torch.cuda.synchronize()
        T.exact(f"{tag}: the phase's render is the render of its start maps", _bits_equal(shp(again, 3), pred))
        ref = bf.fused_grads64(cpu(start), cpu(anchors), pred.cpu(), gs4.cpu(), s64["ratio"], s64["sr"], jac.cpu(), part, SD)
        t32, _, _, _, _, _ = bf.torch_composition(torch_loss, start, anchors, pred, gt4, gs4, jac, part, SD, torch.float32, dev)
        for k in bf.KEYS:
            got = shp(ph.g[_NAME[k]], 3 if k == "a" else 1).clone()
            T.bounded(f"{tag} g_{k}", torch.where(ex.to(dev).expand_as(got), ref[k].float().to(dev), got), ref[k], t32[k])
            raw, (lo, hi) = start[k], bf.LIMS[k]
            outside = (raw < lo) | (raw > hi)
            T.exact(f"{tag} g_{k}: gates", bool(outside.any()) and bool((got[outside] == 0).all()))
            now = shp(ph.p[_NAME[k]], 3 if k == "a" else 1)
            if k not in part:
                T.exact(f"{tag}: {k} is not in the part and stays bit-unchanged", _bits_equal(now, start[k]) and bool((ph.m[_NAME[k]] == 0).all()) and bool((ph.v[_NAME[k]] == 0).all()))
                continue
            # Adam, fed with the gradient the kernel wrote
            m_got, v_got = shp(ph.m[_NAME[k]], now.shape[-1]), shp(ph.v[_NAME[k]], now.shape[-1])
            if t == 1:
                T.exact(f"{tag} m_{k} == (1 - 0.9f) g, bit for bit", _bits_equal(m_got, got * torch.tensor(ONE_MINUS_B1, dtype=torch.float32, device=dev)))
            p64, m64[k], v64[k] = bf.adam64(start[k].cpu(), got.cpu(), m64[k], v64[k], ph.lr_at(t - 1), t, B1, B2)
            p32, m32[k], v32[k] = bf.adam64(start[k], got, m32[k], v32[k], ph.lr_at(t - 1), t, B1, B2, dtype=torch.float32, device=dev)
            T.bounded(f"{tag} adam m_{k}", m_got, m64[k], m32[k])
            T.bounded(f"{tag} adam v_{k}", v_got, v64[k], v32[k])
            T.bounded(f"{tag} adam p_{k} (units of lr)", now, p64, p32, scale=LR)
            big = ~outside & (got.abs() > 1e-6)           # Adam's first step is lr g / (|g| + 1e-8)
            T.exact(f"{tag} p_{k}: the first step moves by Adam's step inside the clamp range and leaves the rest bit-unchanged",
                    t > 1 or (bool(((now - start[k]).abs()[big] > 0.5 * LR).all()) and _bits_equal(now[outside], start[k][outside])))     # (t = 2: momentum moves on)
        if t == 1:
            g_first = {k: ph.g[_NAME[k]].clone() for k in part}
        else:
            T.exact(f"{tag}: the second gradient differs from the first", all(not torch.equal(g_first[k], ph.g[_NAME[k]]) for k in part))
    T.done()


# ------------------------------------------------------------------------------------------------------------------------------
# f. matpbr_brdf_normal_step, called directly, and NormalBrdfPhase once
# ------------------------------------------------------------------------------------------------------------------------------
def _zero_mask(inp):
    B, H, W = inp["B"], inp["H"], inp["W"]
    z = torch.zeros(B, H * W, dtype=torch.bool)
    for b, i in enumerate(inp["zero_pix"]):
        z[b, i] = True
    return z.reshape(B, H, W, 1)


def _normal_step(dev, g, part, st, t=1, lr=LR):
    """One matpbr_brdf_normal_step on fresh buffers: returns the buffers (parameters are copies of the inputs, every output starts as NaN)."""
    from materialist_amd import _lib as L, ops

    B, H, W = g["B"], g["H"], g["W"]
    shapes = {"a": (B, H, W, 3), "r": (B, H, W, 1), "m": (B, H, W, 1), "n": (B, H, W, 3)}
    buf = dict(p={k: (g["pn"] if k == "n" else g["maps"][k]).clone() for k in "armn"}, c={k: _Out(dev, *shapes[k]) for k in "armn"},
               m={k: torch.zeros(shapes[k], device=dev) for k in "armn"}, v={k: torch.zeros(shapes[k], device=dev) for k in "armn"},
               best={k: _Out(dev, *shapes[k]) for k in "armn"}, best_img=_Out(dev, B, H, W, 3), ln=_Out(dev, B, (H * W + 255) // 256))
    ns = L.MatpbrNormalStep()
    for i, k in enumerate("armn"):
        setattr(ns, "p" + k, _P(buf["p"][k]))
        setattr(ns, "c" + k, _P(buf["c"][k].t))
        setattr(ns, "d_" + k, _P(g["d"][k]))
        setattr(ns, k + "0", _P(g["n0"] if k == "n" else g["anchors"][k]))
        setattr(ns, "best_" + k, _P(buf["best"][k].t))
        ns.adam_m[i], ns.adam_v[i] = buf["m"][k].data_ptr(), buf["v"][k].data_ptr()
    ns.best_img, ns.pred, ns.stats, ns.ln_part = _P(buf["best_img"].t), _P(g["pred_z"]), _P(st), _P(buf["ln"].t)
    ns.H, ns.W, ns.batch, ns.part_mask, ns.scale_delta = H, W, B, ops.part_mask(part), SD
    with torch.cuda.device(dev):
        code = _lib().matpbr_brdf_normal_step(ctypes.byref(ns), t, lr, _stream(dev))
    assert code == 0, code
    torch.cuda.synchronize()
    return buf


@pytest.mark.parametrize("part", ["n", "rn", "armn"])
@pytest.mark.parametrize("shape", [(1, 5, 7), (1, 1, 257), (3, 33, 37)], ids=["1x5x7", "1x1x257", "3x33x37"])
def test_normal_step_matches_fp64(shape, part, inputs):
    """The gradient the step hands to Adam (read back as adam_m / (1 - 0.9f) after t = 1) against normal_step_grads64: regularisers, clamp
    gates, NF.normalize's backward with its all-zero vector; the parameters against adam64; the maps of the next render; the normal
    regulariser's per-workgroup sums; the snapshots."""
    dev = _cuda()
    inp = inputs[shape]
    g = _to(dev, inp)
    B, H, W = shape
    T = _Tally()
    s64 = bf.stats64(inp["pred_z"], inp["gt"], inp["maps"], inp["anchors"], part, SD, inp["gt_srgb"])
    st = _row(dev, B, s64, improved=1.0, best=s64["mse"].float())
    buf = _normal_step(dev, g, part, st)
    ref = bf.normal_step_grads64(inp["maps"], inp["anchors"], inp["d"], inp["pn"], inp["n0"], part, SD)
    t32 = bf.normal_step_grads64(g["maps"], g["anchors"], g["d"], g["pn"], g["n0"], part, SD, dtype=torch.float32, device=dev)
    zero = _zero_mask(inp)
    c32 = bf.clamped(g["maps"], torch.float32, dev)
    tag = f"normal_step part '{part}'"
    for k in "armn":
        raw = g["pn"] if k == "n" else g["maps"][k]
        if k not in part:
            T.exact(f"{tag}: {k} is not in the part: parameters, moments and render map untouched",
                    _bits_equal(buf["p"][k], raw) and bool((buf["m"][k] == 0).all()) and bool((buf["v"][k] == 0).all()) and buf["c"][k].all_nan())
            continue
        applied = buf["m"][k].double().cpu() / ONE_MINUS_B1
        p64, _, _ = bf.adam64(raw.cpu(), applied, torch.zeros_like(applied), torch.zeros_like(applied), LR, 1, B1, B2)
        p32, _, _ = bf.adam64(raw, applied.float().to(dev), torch.zeros_like(raw), torch.zeros_like(raw), LR, 1, B1, B2, dtype=torch.float32, device=dev)
        if k == "n":
            zz = zero.expand_as(applied)
            for name, sel in (("the all-zero vectors", zz), ("the other pixels", ~zz)):
                T.bounded(f"{tag} applied g_n, {name}", applied[sel], ref[k][sel], t32[k].cpu()[sel])
            T.exact(f"{tag}: the all-zero vectors' outputs are finite", bool(torch.isfinite(buf["p"][k]).all()) and bool(torch.isfinite(buf["v"][k]).all()) and bool(torch.isfinite(buf["c"][k].t).all()))
            nh64, _ = bf.normalize64(buf["p"][k].cpu())
            T.bounded(f"{tag} cn = normalize(new pn)", buf["c"][k].t, nh64, torch.nn.functional.normalize(buf["p"][k], p=2, dim=-1))
        else:
            T.bounded(f"{tag} applied g_{k}", applied, ref[k], t32[k])
            lo, hi = bf.LIMS[k]
            outside = (raw < lo) | (raw > hi)
            T.exact(f"{tag} g_{k}: gates", bool((buf["m"][k][outside] == 0).all()) and bool((buf["m"][k][~outside] != 0).all()))
            T.exact(f"{tag} c{k} = clamp(new p{k})", _bits_equal(buf["c"][k].t, buf["p"][k].clamp(float(np.float32(lo)), hi)))
        T.bounded(f"{tag} adam p_{k} (units of lr)", buf["p"][k], p64, p32, scale=LR)
        T.exact(f"{tag} c{k}: guard row", buf["c"][k].guard_ok())
    # the normal regulariser's sums, and the snapshots
    nh64, _ = bf.normalize64(inp["pn"])
    nh32 = torch.nn.functional.normalize(g["pn"], p=2, dim=-1)
    ln64 = (nh64 - inp["n0"].double()).abs().reshape(B, -1).sum(dim=1)
    T.bounded(f"{tag} ln_part summed", buf["ln"].t.double().sum(dim=1), ln64, (nh32 - g["n0"]).abs().reshape(B, -1).sum(dim=1))
    T.exact(f"{tag} ln_part: guard row", buf["ln"].guard_ok())
    for k in bf.KEYS:
        T.exact(f"{tag} best_{k} = the clamped map", _bits_equal(buf["best"][k].t, c32[k]) and buf["best"][k].guard_ok())
    T.bounded(f"{tag} best_n", buf["best"]["n"].t, nh64, nh32)
    xs_ref = (inp["pred_z"].double() * st[:, 0].cpu().double().reshape(B, 1, 1, 1)).clamp_min(bf.EPS) ** (1.0 / 2.2)
    xs32 = (g["pred_z"] * st[:, 0].reshape(B, 1, 1, 1)).clamp_min(bf.EPS) ** (1.0 / 2.2)
    T.bounded(f"{tag} best_img", buf["best_img"].t, xs_ref, xs32)
    if part == "armn":                   # not improved: the same step, no snapshot; stopped earlier: nothing at all
        st0 = st.clone()
        st0[:, 8] = 0.0
        b0 = _normal_step(dev, g, part, st0)
        T.exact(f"{tag}: improved = 0 leaves the snapshots NaN", all(b0["best"][k].all_nan() for k in "armn") and b0["best_img"].all_nan())
        T.exact(f"{tag}: improved = 0 takes the same step", all(_bits_equal(b0["p"][k], buf["p"][k]) for k in "armn"))
        st0[B - 1, 13] = 2.0
        b1 = _normal_step(dev, g, part, st0)
        T.exact(f"{tag}: an image stopped earlier rests", all(_bits_equal(b1["p"][k][B - 1], (g["pn"] if k == "n" else g["maps"][k])[B - 1]) for k in "armn") and
                bool(torch.isnan(b1["ln"].t[B - 1]).all()) and (B == 1 or all(_bits_equal(b1["p"][k][:B - 1], buf["p"][k][:B - 1]) for k in "armn")))
    T.done()


def test_normal_phase_applies_the_fp64_gradients():
    """NormalBrdfPhase once at 16 x 16, part 'armn': after one step adam_m / (1 - 0.9f) against normal_step_grads64 fed with the phase's own
    backward-render gradients `g`, and its statistics row against stats64 of its own render."""
    from materialist_amd import loop, render

    dev = _cuda()
    B, H, W = 1, 16, 16
    spp = 8
    depth, light, init, true = _scene_inputs(dev, B, H, W, 50)
    geo = render.load_estimated_mesh(depth, use_mesh_normal=True).shading_normal()
    gen = torch.Generator(device="cpu").manual_seed(11)
    n_true = torch.nn.functional.normalize(geo + 0.2 * torch.randn(geo.shape, generator=gen).to(dev), dim=-1).contiguous()
    n_init = (1.7 * torch.nn.functional.normalize(geo + 0.1 * torch.randn(geo.shape, generator=gen).to(dev), dim=-1)).contiguous()
    n_orig = torch.nn.functional.normalize(geo + 0.05 * torch.randn(geo.shape, generator=gen).to(dev), dim=-1).contiguous()

    def make_scene():
        s = render.load_estimated_mesh(depth, use_mesh_normal=False)
        s._set("emitter.data", light)
        return s

    with torch.no_grad():
        gt = render.render_w_brdf(make_scene(), *true, n_true, spp)
    originals = {"albedo": (init[0] * 0.9).clamp(0.02, 0.98), "roughness": (init[1] * 0.9).clamp(0.1, 0.9), "metallic": (init[2] * 0.9 + 0.02).clamp(0.02, 0.9),
                 "normal": n_orig}
    ph = loop.NormalBrdfPhase(make_scene(), gt, *init, n_init, optimize_part="armn", spp=spp, lr=LR, originals=originals)
    shp = lambda t, c: t.reshape(B, H, W, c)
    chan = {"a": 3, "r": 1, "m": 1, "n": 3}
    start = {k: shp(ph.p[_NAME[k]], chan[k]).clone() for k in "armn"}
    ph.step()
    torch.cuda.synchronize()
    anchors = {k: shp(ph.orig[_NAME[k]], chan[k]) for k in "armn"}
    d = {k: shp(ph.g[_NAME[k]], chan[k]) for k in "armn"}
    cpu = lambda x: {k: v.cpu() for k, v in x.items()}
    T = _Tally()
    s64 = bf.stats64(shp(ph.pred, 3).cpu(), shp(ph.gt, 3).cpu(), cpu(start), cpu(anchors), "armn", SD, shp(ph.gt_srgb, 3).cpu())
    s32 = bf.stats64(shp(ph.pred, 3), shp(ph.gt, 3), start, anchors, "armn", SD, shp(ph.gt_srgb, 3), dtype=torch.float32, device=dev)
    row = ph.stats.cpu()
    for i, k in enumerate(bf.SLOTS):
        T.bounded(f"normal phase stats {k}", row[:, i], s64[k], s32[k])
    ref = bf.normal_step_grads64(cpu(start), cpu(anchors), cpu(d), start["n"].cpu(), anchors["n"].cpu(), "armn", SD)
    t32 = bf.normal_step_grads64(start, anchors, d, start["n"], anchors["n"], "armn", SD, dtype=torch.float32, device=dev)
    for k in "armn":
        applied = shp(ph.m[_NAME[k]], chan[k]).double().cpu() / ONE_MINUS_B1
        T.bounded(f"normal phase applied g_{k}", applied, ref[k], t32[k])
        p64, _, _ = bf.adam64(start[k].cpu(), applied, torch.zeros_like(applied), torch.zeros_like(applied), ph.lr_at(0), 1, B1, B2)
        p32, _, _ = bf.adam64(start[k], applied.float().to(dev), torch.zeros_like(start[k]), torch.zeros_like(start[k]), ph.lr_at(0), 1, B1, B2, dtype=torch.float32,
                              device=dev)
        T.bounded(f"normal phase adam p_{k} (units of lr)", shp(ph.p[_NAME[k]], chan[k]), p64, p32, scale=LR)
    T.done()
