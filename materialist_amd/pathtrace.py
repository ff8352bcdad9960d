"""Path-traced re-render of the depth mesh: the ctypes binding of libmatpbr_path.so (include/matpbr_path.h) and `PathTracer`.

The deterministic render is direct light, unshadowed, under SH25.  The reference's *final* images come from
Mitsuba's `path` integrator, `max_depth` 4, on the `.ply` mesh under the texel envmap (render_final.py:35-96, inverse_img_w_mi.py:
49-52).  `PathTracer` is that render on the GPU: shadows, inter-reflection, the envmap's texels as the light.
Forward only: no autograd.  There is no fallback: a missing or failing library raises.
"""
from __future__ import annotations

import ctypes
import threading
import time
from typing import Dict, Optional

import numpy as np
import torch

from . import build as _build

_P = ctypes.c_void_p
_lib = None
_lock = threading.Lock()

NODE_BYTES = 64
TRI_BYTES = 48
MAX_BVH_DEPTH = 40

SIGNATURES = {
    "matpbr_path_version": (ctypes.c_int, []),
    "matpbr_path_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "matpbr_path_bvh_size": (ctypes.c_int, [ctypes.c_long, _P]),
    "matpbr_path_bvh_build": (ctypes.c_int, [_P, ctypes.c_long, _P, ctypes.c_long, _P, ctypes.c_long, _P, _P, _P, _P]),
    "matpbr_path_trace_host": (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_long, ctypes.c_float, ctypes.c_float, _P, _P]),
    "matpbr_path_env_tables": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, _P, _P, _P, _P]),
    "matpbr_path_env_sample_host": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, ctypes.c_long, _P, _P, _P]),
    "matpbr_path_render": (ctypes.c_int, [_P] * 5 + [ctypes.c_int, ctypes.c_int, ctypes.c_float] + [_P] * 4 +
                           [ctypes.c_int] * 4 + [ctypes.c_uint32, ctypes.c_int, _P, _P, _P]),
}


class PathError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Load libmatpbr_path.so (building it first when it is missing or older than its sources) and bind every symbol."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        _build.build_path_library()
        lib = ctypes.CDLL(_build.PATH_LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
        return lib


def check(code: int, what: str) -> None:
    if code != 0:
        msg = load().matpbr_path_strerror(code)
        raise PathError(f"{what} failed: {msg.decode() if msg else code} ({code})")


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def build_bvh(vertices: np.ndarray, triangles: np.ndarray) -> Dict[str, object]:
    """Host BVH of a triangle mesh: {"nodes" uint8 [n_nodes*64], "tris" uint8 [T*48], "n_nodes", "depth", "n_leaves", "build_s"}."""
    lib = load()
    V = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    T = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
    cap = ctypes.c_long(0)
    check(lib.matpbr_path_bvh_size(T.shape[0], ctypes.cast(ctypes.byref(cap), _P)), "matpbr_path_bvh_size")
    nodes = np.zeros(cap.value * NODE_BYTES, dtype=np.uint8)
    tris = np.zeros(max(T.shape[0], 1) * TRI_BYTES, dtype=np.uint8)
    n_nodes, depth, n_leaves = ctypes.c_long(0), ctypes.c_int(0), ctypes.c_long(0)
    t0 = time.perf_counter()
    code = lib.matpbr_path_bvh_build(_ptr(V), V.shape[0], _ptr(T), T.shape[0], _ptr(nodes), cap.value, _ptr(tris),
                                     ctypes.cast(ctypes.byref(n_nodes), _P), ctypes.cast(ctypes.byref(depth), _P),
                                     ctypes.cast(ctypes.byref(n_leaves), _P))
    build_s = time.perf_counter() - t0
    check(code, "matpbr_path_bvh_build")
    return {"nodes": nodes[: n_nodes.value * NODE_BYTES].copy(), "tris": tris, "n_nodes": n_nodes.value, "depth": depth.value,
            "n_leaves": n_leaves.value, "build_s": build_s}


def trace_host(bvh: Dict[str, object], origins: np.ndarray, dirs: np.ndarray, tmin: float = 0.0, tmax: float = 3.0e38):
    """Closest hit on the CPU with the kernel's routine -> (t [N] float32, tmax where missed; triangle index [N] int32, -1 = miss)."""
    o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    t = np.empty(o.shape[0], np.float32)
    k = np.empty(o.shape[0], np.int32)
    check(load().matpbr_path_trace_host(_ptr(bvh["nodes"]), _ptr(bvh["tris"]), _ptr(o), _ptr(d), o.shape[0], tmin, tmax, _ptr(t), _ptr(k)),
          "matpbr_path_trace_host")
    return t, k


def env_tables(env: np.ndarray) -> Dict[str, object]:
    """Emitter-sampling tables of an envmap [He,We,3] (fp64 on the host, stored fp32): row_cdf [He+1], col_cdf [He,We+1], pdf [He,We]."""
    E = np.ascontiguousarray(env, dtype=np.float32)
    He, We = E.shape[:2]
    row = np.empty(He + 1, np.float32)
    col = np.empty((He, We + 1), np.float32)
    pdf = np.empty((He, We), np.float32)
    total = ctypes.c_double(0.0)
    check(load().matpbr_path_env_tables(_ptr(E), He, We, _ptr(row), _ptr(col), _ptr(pdf), ctypes.cast(ctypes.byref(total), _P)),
          "matpbr_path_env_tables")
    return {"row_cdf": row, "col_cdf": col, "pdf": pdf, "total": total.value}


def env_sample_host(tables: Dict[str, object], u: np.ndarray):
    """The render's emitter sampler on the CPU: u [N,4] -> (dir [N,3], pdf [N], texel [N] = row*We + col)."""
    U = np.ascontiguousarray(u, dtype=np.float32).reshape(-1, 4)
    He, We = tables["pdf"].shape
    d = np.empty((U.shape[0], 3), np.float32)
    p = np.empty(U.shape[0], np.float32)
    k = np.empty(U.shape[0], np.int32)
    check(load().matpbr_path_env_sample_host(_ptr(tables["row_cdf"]), _ptr(tables["col_cdf"]), _ptr(tables["pdf"]), He, We, _ptr(U), U.shape[0],
                                             _ptr(d), _ptr(p), _ptr(k)), "matpbr_path_env_sample_host")
    return d, p, k


class PathTracer:
    """One mesh in the renderer's frame (camera at the origin looking down -z, `fov_x_deg` horizontal field of view, H x W pixels).
    The BVH is built once on the host and kept on the device; `render` takes the maps and the envmap of each frame."""

    def __init__(self, vertices: np.ndarray, triangles: np.ndarray, H: int, W: int, fov_x_deg: float = 35.0, device="cuda"):
        self.H, self.W, self.fov = int(H), int(W), float(fov_x_deg)
        self.device = torch.device(device)
        bvh = build_bvh(vertices, triangles)
        self.stats = {k: bvh[k] for k in ("n_nodes", "depth", "n_leaves", "build_s")}
        self.stats["n_tris"] = int(np.asarray(triangles).reshape(-1, 3).shape[0])
        self.stats["bytes"] = int(bvh["nodes"].nbytes + bvh["tris"].nbytes)
        self.nodes = torch.from_numpy(bvh["nodes"]).to(self.device)
        self.tris = torch.from_numpy(bvh["tris"]).to(self.device)

    def _tables(self, env: torch.Tensor):
        tab = env_tables(env.cpu().numpy())          # host, fp64 -> fp32: microseconds for the 16 x 32 maps of the pipeline
        return (env.contiguous(), *(torch.from_numpy(np.ascontiguousarray(tab[k])).to(self.device) for k in ("row_cdf", "col_cdf", "pdf")))

    @torch.no_grad()
    def render(self, albedo: torch.Tensor, roughness: torch.Tensor, metallic: torch.Tensor, envmap, spp: int = 64, max_depth: int = 4,
               seed: int = 0, spp_per_launch: int = 8, out: Optional[torch.Tensor] = None, rays: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> linear radiance [H,W,3] on the current torch stream.  albedo [H,W,3], roughness / metallic [H,W] or [H,W,1], envmap
        [He,We,3] (tensor or array, the `sh.py` equirectangular convention).  Every split into launches of `spp_per_launch` samples gives
        the same bits.  `rays` (optional int32 [H,W] on the device): the rays each pixel traced are added to it."""
        H, W, dev = self.H, self.W, self.device
        f = lambda x, c: torch.as_tensor(x).to(dev, torch.float32).reshape(H, W, c).contiguous()
        a, r, m = f(albedo, 3), f(roughness, 1), f(metallic, 1)
        env = torch.as_tensor(envmap).to(dev, torch.float32)
        if env.dim() != 3 or env.shape[2] != 3:
            raise ValueError(f"envmap must be [He,We,3], got {tuple(env.shape)}")
        env, row, col, pdf = self._tables(env)
        if out is None:
            out = torch.empty(H, W, 3, device=dev, dtype=torch.float32)
        stream = torch.cuda.current_stream(dev).cuda_stream
        lib = load()
        code = lib.matpbr_path_render(self.nodes.data_ptr(), self.tris.data_ptr(), a.data_ptr(), r.data_ptr(), m.data_ptr(), H, W, self.fov,
                                      env.data_ptr(), row.data_ptr(), col.data_ptr(), pdf.data_ptr(), int(env.shape[0]), int(env.shape[1]),
                                      int(spp), int(max_depth), int(seed) & 0xFFFFFFFF, int(spp_per_launch), out.data_ptr(),
                                      rays.data_ptr() if rays is not None else None, stream)
        check(code, "matpbr_path_render")
        return out
