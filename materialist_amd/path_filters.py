"""The image-space steps around the path render: the a-trous denoiser ("Denoiser"), the differential render's
composite ("Differential render", "Ratio shadow transfer", "Material edits in the photograph"), the quotient composite ("Relighting in the
photograph") and the differential render's own denoiser ("Denoiser for the differential render").  Each step is written once, over a
side: `_HOST` runs it on numpy arrays through the library's `*_host` entry (the routine the kernel runs, for the tests), `_Device`
on torch tensors through the kernel on the current torch stream.  The public `NAME_host` and `NAME` are the two calls of that body."""
from itertools import chain
from typing import Optional

import numpy as np
import torch

from .path_abi import DENOISE_DEFAULTS, PathDenoise, _ptr, _ref, check, symbol
from .path_host import _host_image


def denoise_params(levels: Optional[int] = None, sigma_n: Optional[float] = None, sigma_x: Optional[float] = None,
                   sigma_a: Optional[float] = None, sigma_c: Optional[float] = None) -> PathDenoise:
    """The filter's parameters (None: DENOISE_DEFAULTS), checked as the library checks them; ValueError when bad."""
    given = {"levels": levels, "sigma_n": sigma_n, "sigma_x": sigma_x, "sigma_a": sigma_a, "sigma_c": sigma_c}
    v = {k: DENOISE_DEFAULTS[k] if x is None else x for k, x in given.items()}
    if int(v["levels"]) != v["levels"] or not 1 <= int(v["levels"]) <= 8:
        raise ValueError(f"levels must be an integer in 1..8, got {v['levels']}")
    for k in ("sigma_n", "sigma_x", "sigma_a", "sigma_c"):
        if not (float(v[k]) > 0 and np.isfinite(float(v[k]))):
            raise ValueError(f"{k} must be positive and finite, got {v[k]}")
    return PathDenoise(int(v["levels"]), float(v["sigma_n"]), float(v["sigma_x"]), float(v["sigma_a"]), float(v["sigma_c"]))


def _device_of(*xs):
    """The device of the first CUDA tensor among `xs` (a tuple or list among them stands for its members); "cuda" when there is none."""
    for x in xs:
        for y in x if isinstance(x, (tuple, list)) else (x,):
            if isinstance(y, torch.Tensor) and y.is_cuda:
                return y.device
    return torch.device("cuda")


class _Host:
    """The CPU side of a step: numpy arrays, the library's entry of the step's name + "_host", no stream."""
    suffix, raw, ptr, tail = "_host", staticmethod(np.asarray), staticmethod(_ptr), ()

    def images(self, specs) -> list:
        """The images of `specs`, (x, shape, what) each, checked and converted in order."""
        return [_host_image(x, shape, what) for x, shape, what in specs]

    def empty(self, *shape) -> np.ndarray:
        return np.empty(shape, np.float32)

    def workspace(self, nbytes: int, given=None) -> np.ndarray:
        return np.empty(nbytes // 4, np.float32)


class _Device:
    """The device side of a step: torch tensors on the device of the first CUDA tensor among `where` ("cuda" without one), the kernel's
    entry, the current torch stream last (`images` finds both).  Every shape is checked before the first image moves: a refusal touches
    no device."""
    suffix, raw, ptr = "", staticmethod(torch.as_tensor), staticmethod(torch.Tensor.data_ptr)

    def __init__(self, *where):
        self.where = where

    def images(self, specs) -> list:
        checked = []
        for x, shape, what in specs:
            t = torch.as_tensor(x)
            if t.shape != shape:
                raise ValueError(f"{what} must be {list(shape)}, got {list(t.shape)}")
            checked.append(t)
        dev = self.dev = _device_of(*self.where)
        self.tail = (torch.cuda.current_stream(dev).cuda_stream,)
        return [t.to(dev, torch.float32).contiguous() for t in checked]

    def empty(self, *shape) -> torch.Tensor:
        return torch.empty(*shape, device=self.dev, dtype=torch.float32)

    def workspace(self, nbytes: int, given: Optional[torch.Tensor] = None) -> torch.Tensor:
        if given is None or given.numel() * given.element_size() < nbytes:
            given = torch.empty(nbytes, device=self.dev, dtype=torch.uint8)
        return given


_HOST = _Host()


def _run(side, name: str, ins, scalars, outs, *last) -> None:
    """The step `name` on `side`: the addresses of the arrays `ins`, the `scalars`, the addresses of the arrays `outs`, what is `last`,
    and the side's tail (the stream)."""
    name += side.suffix
    check(symbol(name)(*map(side.ptr, ins), *scalars, *map(side.ptr, outs), *last, *side.tail), name)


def _geom_shape(geom, what: str = "geom") -> tuple:
    shp = tuple(geom.shape)
    if len(shp) != 3 or shp[2] != 8 or shp[0] < 1 or shp[1] < 1:
        raise ValueError(f"{what} must be [H,W,8], got {list(shp)}")
    return shp[0], shp[1]


# ---- the denoiser ("Denoiser") ----------------------------------------------------------------------------------
def _denoise_prepare(side, A, B, geom):
    H, W = _geom_shape(side.raw(geom))
    a, b, g = side.images([(A, (H, W, 3), "A"), (B, (H, W, 3), "B"), (geom, (H, W, 8), "geom")])
    cv = side.empty(H, W, 4)
    _run(side, "matpbr_path_denoise_prepare", (a, b, g), (H, W), (cv,))
    return cv


def denoise_prepare_host(A: np.ndarray, B: np.ndarray, geom: np.ndarray) -> np.ndarray:
    """The filter's first step on the CPU with the routine the kernel runs: A, B [H,W,3], geom [H,W,8] -> cv0 [H,W,4] = ((A + B) / 2,
    the prefiltered variance of the mean's luminance)."""
    return _denoise_prepare(_HOST, A, B, geom)


@torch.no_grad()
def denoise_prepare(A, B, geom) -> torch.Tensor:
    """`denoise_prepare_host` on the device (the current torch stream) -> cv0 [H,W,4]."""
    return _denoise_prepare(_Device(geom, A, B), A, B, geom)


def _level(side, name: str, cv, cov, geom, alb, level, params):
    """One a-trous level through `name`; `cov`: the differential filter's coverage, which follows cv, or None."""
    prm = denoise_params(**params)
    H, W = _geom_shape(side.raw(geom))
    if not 0 <= int(level) <= 7:
        raise ValueError(f"level must lie in 0..7, got {level}")
    specs = [(cv, (H, W, 4), "cv"), (cov, (H, W), "cov"), (geom, (H, W, 8), "geom"), (alb, (H, W, 3), "alb")]
    ins = side.images(specs if cov is not None else specs[:1] + specs[2:])
    out = side.empty(H, W, 4)
    _run(side, name, ins, (H, W, _ref(prm), int(level)), (out,))
    return out


def denoise_level_host(cv: np.ndarray, geom: np.ndarray, alb: np.ndarray, level: int, **params) -> np.ndarray:
    """One a-trous level (stride 2^level) on the CPU with the routine the kernel runs: cv [H,W,4], geom [H,W,8], alb [H,W,3] ->
    cv [H,W,4].  `params`: levels, sigma_n, sigma_x, sigma_a, sigma_c (`denoise_params`)."""
    return _level(_HOST, "matpbr_path_denoise_level", cv, None, geom, alb, level, params)


@torch.no_grad()
def denoise_level(cv, geom, alb, level: int, **params) -> torch.Tensor:
    """`denoise_level_host` on the device (the current torch stream) -> cv [H,W,4]."""
    return _level(_Device(geom, cv, alb), "matpbr_path_denoise_level", cv, None, geom, alb, level, params)


@torch.no_grad()
def denoise(A, B, alb, geom, workspace: Optional[torch.Tensor] = None, **params) -> torch.Tensor:
    """The whole filter on the device (the current torch stream): two half renders A, B [H,W,3], the albedo guide alb [H,W,3] and the
    features geom [H,W,8] -> the denoised mean [H,W,3].  Equal to `denoise_prepare` and `levels` calls of `denoise_level`, bit for
    bit.  `workspace`: a uint8 device tensor of at least matpbr_path_denoise_workspace_bytes (default: allocated here)."""
    side = _Device(geom, A, B, alb)
    prm = denoise_params(**params)
    H, W = _geom_shape(side.raw(geom))
    a, b, al, g = side.images([(A, (H, W, 3), "A"), (B, (H, W, 3), "B"), (alb, (H, W, 3), "alb"), (geom, (H, W, 8), "geom")])
    nbytes = int(symbol("matpbr_path_denoise_workspace_bytes")(H, W))
    out = side.empty(H, W, 3)
    _run(side, "matpbr_path_denoise", (a, b, g, al), (H, W, _ref(prm)), (out, side.workspace(nbytes, workspace)), nbytes)
    return out


# ---- the differential render's composite ("Differential render") -------------------------------------------------
def _composite_scale(scale: float) -> float:
    sc = float(scale)
    if not (np.isfinite(np.float32(sc)) and np.float32(sc) > 0):
        raise ValueError(f"scale must be finite and positive (1 / the number of frames summed), got {scale}")
    return sc


def _composite(side, fg, delta, alpha, photo, scale, base=None):
    """`composite`; with `base`, `composite_ratio`: the entry of that name takes it after delta."""
    shp = tuple(side.raw(photo).shape)
    if len(shp) != 3 or shp[2] != 3 or shp[0] < 1 or shp[1] < 1:
        raise ValueError(f"photo must be [H,W,3], got {list(shp)}")
    H, W = shp[:2]
    sc = _composite_scale(scale)
    specs = [(fg, (H, W, 3), "fg"), (delta, (H, W, 3), "delta"), (base, (H, W, 3), "base"), (alpha, (H, W), "alpha"), (photo, (H, W, 3), "photo")]
    images = side.images(specs if base is not None else specs[:2] + specs[3:])
    out = side.empty(H, W, 3)
    _run(side, "matpbr_path_composite" + ("_ratio" if base is not None else ""), images, (H, W, sc), (out,))
    return out


def composite_host(fg, delta, alpha, photo, scale: float = 1.0) -> np.ndarray:
    """`composite` on the CPU with the routine the kernel runs: fg, delta, photo [H,W,3], alpha [H,W] -> [H,W,3], the same bits."""
    return _composite(_HOST, fg, delta, alpha, photo, scale)


@torch.no_grad()
def composite(fg, delta, alpha, photo, scale: float = 1.0) -> torch.Tensor:
    """The differential render composited into the photograph, on the device (the current torch stream): max(0, (fg + delta) scale +
    (1 - alpha scale) photo) per channel, every operation rounded on its own.  fg, delta, alpha: `PathTracer.render_diff`'s outputs,
    or their sums over some frames with `scale` = 1 / (the number of frames); photo [H,W,3], linear.  Where fg, delta and alpha are 0
    the photograph (>= 0) comes through bit for bit."""
    return _composite(_Device(fg, delta, alpha, photo), fg, delta, alpha, photo, scale)


def _ratio_base(base):
    if base is None:
        raise ValueError("base must be [H,W,3], got None")
    return base


def composite_ratio_host(fg, delta, base, alpha, photo, scale: float = 1.0) -> np.ndarray:
    """`composite_ratio` on the CPU with the routine the kernel runs: fg, delta, base, photo [H,W,3], alpha [H,W] -> [H,W,3], the same
    bits."""
    return _composite(_HOST, fg, delta, alpha, photo, scale, _ratio_base(base))


@torch.no_grad()
def composite_ratio(fg, delta, base, alpha, photo, scale: float = 1.0) -> torch.Tensor:
    """The differential render composited into the photograph with its shadows transferred as a ratio ("Ratio
    shadow transfer"), on the device (the current torch stream).  fg, delta, base, alpha: `PathTracer.render_diff_ratio`'s outputs, or
    their sums over some frames with `scale` = 1 / (the number of frames); photo [H,W,3], linear.  Per channel, where delta < 0 < base
    (the objects darken it) the photograph's share is multiplied by g = max(0, base + delta) / base: max(0, fg scale + ((1 - alpha
    scale) photo) g); elsewhere the channel carries `composite`'s bits.  Where fg, delta and alpha are 0 the photograph (>= 0) comes
    through bit for bit."""
    return _composite(_Device(fg, delta, base, alpha, photo), fg, delta, alpha, photo, scale, _ratio_base(base))


def _composite_edit(side, zeros, delta, photo, base):
    """`composite` (with `base`, `composite_ratio`) of a differential render without inserted objects: fg and alpha are zeros of the
    photograph's frame, made by `zeros(shape)` once every shape is known to be right."""
    shp = tuple(side.raw(photo).shape)
    if len(shp) != 3 or shp[2] != 3 or shp[0] < 1 or shp[1] < 1:
        raise ValueError(f"photo must be [H,W,3], got {list(shp)}")
    for x, what in ((delta, "delta"), (base, "base")):
        if x is not None and tuple(side.raw(x).shape) != shp:
            raise ValueError(f"{what} must be {list(shp)}, got {list(side.raw(x).shape)}")
    return _composite(side, zeros(shp), delta, zeros(shp[:2]), photo, 1.0, base)


def composite_edit_host(delta, photo, base=None) -> np.ndarray:
    """`composite_edit` on the CPU with the routines the kernels run -> [H,W,3], the same bits."""
    return _composite_edit(_HOST, lambda s: np.zeros(s, np.float32), delta, photo, base)


@torch.no_grad()
def composite_edit(delta, photo, base=None) -> torch.Tensor:
    """`PathTracer.render_edit_diff`'s outputs composited into the photograph ("Material edits in the
    photograph"), on the device: `composite` with fg and alpha zero, max(0, photo + delta) (additive); with `base`, `composite_ratio`
    with them zero: where the edit darkens a channel (delta < 0 < base) the photograph is multiplied by max(0, base + delta) / base, so
    the fit's albedo cancels.  Where delta is 0 the photograph (>= 0) comes through bit for bit."""
    where = (delta, photo) if base is None else (delta, photo, base)
    return _composite_edit(_Device(*where), lambda s: torch.zeros(s, dtype=torch.float32, device=_device_of(*where)), delta, photo, base)


# ---- the quotient composite ("Relighting in the photograph") -----------------------------------------------------
RELIGHT_FLOOR = 0.01   # the default floor over the frame's mean model radiance: where a channel is that dark the ratio starts to give way


def _composite_relight(side, base, relit, photo, scale, floor):
    shp = tuple(side.raw(photo).shape)
    if len(shp) != 3 or shp[2] != 3 or shp[0] < 1 or shp[1] < 1:
        raise ValueError(f"photo must be [H,W,3], got {list(shp)}")
    H, W = shp[:2]
    sc = _composite_scale(scale)
    if floor is not None and not (np.isfinite(np.float32(floor)) and np.float32(floor) > 0):
        raise ValueError(f"floor must be finite and positive, got {floor}")
    b, r, p = side.images([(base, (H, W, 3), "base"), (relit, (H, W, 3), "relit"), (photo, (H, W, 3), "photo")])
    if floor is None:   # in fp64 over all pixels and channels, then one rounding to float32
        mean = float(b.mean(dtype=np.float64)) if isinstance(b, np.ndarray) else float(b.double().mean())
        floor = float(np.float32(RELIGHT_FLOOR * sc * mean))
        if not (np.isfinite(floor) and floor > 0):
            raise ValueError(f"the default floor is {RELIGHT_FLOOR} x mean(base scale) = {floor}: base has no light to take a ratio over; pass floor")
    out = side.empty(H, W, 3)
    _run(side, "matpbr_path_composite_relight", (b, r, p), (H, W, sc, float(floor)), (out,))
    return out


def composite_relight_host(base, relit, photo, scale: float = 1.0, floor: Optional[float] = None) -> np.ndarray:
    """`composite_relight` on the CPU with the routine the kernel runs: base, relit, photo [H,W,3] -> [H,W,3], the same bits for the
    same `floor`."""
    return _composite_relight(_HOST, base, relit, photo, scale, floor)


@torch.no_grad()
def composite_relight(base, relit, photo, scale: float = 1.0, floor: Optional[float] = None) -> torch.Tensor:
    """`PathTracer.render_relight`'s outputs composited into the photograph ("Relighting in the photograph"),
    on the device (the current torch stream): the quotient image max(0, photo g), g = (relit scale + floor) / (base scale + floor) per
    channel, every operation rounded on its own.  base, relit: the radiance under the fitted and under the new light, or their sums
    over some frames with `scale` = 1 / (the number of frames); photo [H,W,3], linear.  `floor` > 0 bounds g where the model is
    dark; None: RELIGHT_FLOOR (0.01) x the mean of base scale over all pixels and channels.  Where relit has base's bits the
    photograph (>= 0) comes through bit for bit."""
    return _composite_relight(_Device(base, relit, photo), base, relit, photo, scale, floor)


# ---- the differential render's denoiser ("Denoiser for the differential render") ----------------------------------
# A, B: the (fg [H,W,3], delta [H,W,3], alpha [H,W]) triples of two sums of `PathTracer.render_diff`'s outputs over the same number of
# frames, with independent seeds and equal spp; scale = 1 / (frames summed per half).
def _halves(A, B, H: int, W: int):
    """The six images of two triples as `images` takes them, in the library's order.  A generator: the triples are looked at when the
    images before them in a chain have been checked."""
    if len(A) != 3 or len(B) != 3:
        raise ValueError("A and B must be (fg, delta, alpha) triples")
    for name, t in (("A", A), ("B", B)):
        for k, x in enumerate(t):
            yield x, (H, W, 3) if k < 2 else (H, W), f"{name}[{k}] ({('fg', 'delta', 'alpha')[k]})"


def _denoise_diff_prepare(side, A, B, geom, scale):
    H, W = _geom_shape(side.raw(geom))
    sc = _composite_scale(scale)
    *hs, g = side.images(chain(_halves(A, B, H, W), [(geom, (H, W, 8), "geom")]))
    cv, cov = side.empty(H, W, 4), side.empty(H, W)
    _run(side, "matpbr_path_denoise_diff_prepare", (*hs, g), (H, W, sc), (cv, cov))
    return cv, cov


def denoise_diff_prepare_host(A, B, geom, scale: float = 1.0) -> tuple:
    """The filter's first step on the CPU with the routine the kernel runs -> (cv0 [H,W,4], cov [H,W]): the own layer's unpremultiplied
    mean with the prefiltered variance of its luminance, and the own layer's coverage."""
    return _denoise_diff_prepare(_HOST, A, B, geom, scale)


@torch.no_grad()
def denoise_diff_prepare(A, B, geom, scale: float = 1.0) -> tuple:
    """`denoise_diff_prepare_host` on the device (the current torch stream) -> (cv0 [H,W,4], cov [H,W])."""
    return _denoise_diff_prepare(_Device(geom, A, B), A, B, geom, scale)


def denoise_diff_level_host(cv, cov, geom, alb, level: int, **params) -> np.ndarray:
    """One a-trous level of the differential render's filter on the CPU with the routine the kernel runs -> cv [H,W,4]."""
    return _level(_HOST, "matpbr_path_denoise_diff_level", cv, cov, geom, alb, level, params)


@torch.no_grad()
def denoise_diff_level(cv, cov, geom, alb, level: int, **params) -> torch.Tensor:
    """`denoise_diff_level_host` on the device (the current torch stream) -> cv [H,W,4]."""
    return _level(_Device(geom, cv, cov, alb), "matpbr_path_denoise_diff_level", cv, cov, geom, alb, level, params)


def _denoise_diff_finish(side, cv, cov, A, B, geom, scale):
    H, W = _geom_shape(side.raw(geom))
    sc = _composite_scale(scale)
    c, k, g, *hs = side.images(chain([(cv, (H, W, 4), "cv"), (cov, (H, W), "cov"), (geom, (H, W, 8), "geom")], _halves(A, B, H, W)))
    outs = side.empty(H, W, 3), side.empty(H, W, 3), side.empty(H, W)
    _run(side, "matpbr_path_denoise_diff_finish", (c, k, *hs, g), (H, W, sc), outs)
    return outs


def denoise_diff_finish_host(cv, cov, A, B, geom, scale: float = 1.0) -> tuple:
    """The filter's last step on the CPU with the routine the kernel runs -> (fg', delta', alpha'): the own layer's filtered colour times
    its coverage, the other layer's mean and the mean alpha as they are."""
    return _denoise_diff_finish(_HOST, cv, cov, A, B, geom, scale)


@torch.no_grad()
def denoise_diff_finish(cv, cov, A, B, geom, scale: float = 1.0) -> tuple:
    """`denoise_diff_finish_host` on the device (the current torch stream) -> (fg', delta', alpha')."""
    return _denoise_diff_finish(_Device(geom, cv, cov, A, B), cv, cov, A, B, geom, scale)


def _denoise_diff(side, A, B, alb, geom, scale, workspace, params):
    prm = denoise_params(**params)
    H, W = _geom_shape(side.raw(geom))
    sc = _composite_scale(scale)
    *hs, al, g = side.images(chain(_halves(A, B, H, W), [(alb, (H, W, 3), "alb"), (geom, (H, W, 8), "geom")]))
    nbytes = int(symbol("matpbr_path_denoise_diff_workspace_bytes")(H, W))
    outs = side.empty(H, W, 3), side.empty(H, W, 3), side.empty(H, W)
    _run(side, "matpbr_path_denoise_diff", (*hs, g, al), (H, W, sc, _ref(prm)), (*outs, side.workspace(nbytes, workspace)), nbytes)
    return outs


def denoise_diff_host(A, B, alb, geom, scale: float = 1.0, **params) -> tuple:
    """`denoise_diff` on the CPU with the routines the kernels run -> (fg', delta', alpha').  Equal to its separate steps bit for bit."""
    return _denoise_diff(_HOST, A, B, alb, geom, scale, None, params)


@torch.no_grad()
def denoise_diff(A, B, alb, geom, scale: float = 1.0, workspace: Optional[torch.Tensor] = None, **params) -> tuple:
    """The differential render's filter on the device (the current torch stream): the triples A and B, the albedo guide alb [H,W,3] and
    the features geom [H,W,8] -> (fg', delta', alpha'), which `composite(fg', delta', alpha', photo, 1.0)` puts into the photograph.
    Equal to `denoise_diff_prepare`, `levels` calls of `denoise_diff_level` and `denoise_diff_finish`, bit for bit.  `workspace`: a uint8
    device tensor of at least matpbr_path_denoise_diff_workspace_bytes (default: allocated here)."""
    return _denoise_diff(_Device(geom, alb, A, B), A, B, alb, geom, scale, workspace, params)
