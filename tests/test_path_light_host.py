"""Host side of emissive inserted objects ("Emissive inserted objects"): the exported symbols, the emitter
choice, the area sampler and both pdfs the kernel runs (on the CPU), the light tables against fp64 numpy, the C ABI's refusals, the
fp64 restatement `path_objects_fp64.replay_objects` against closed forms (Lambert's polygon formula, the furnace box) and against
the recorded PBR restatement, over the library's fp32 traversal, and the routing of `merge_objects` / `load_oi_scene`.  No GPU needed."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import path_fp64 as pf  # noqa: E402
import path_light_fp64 as pl  # noqa: E402
import path_objects_fp64 as pob  # noqa: E402
import path_oi_fp64 as po  # noqa: E402
import path_oi_pbr_fp64 as pp  # noqa: E402
import path_testlib as tl  # noqa: E402

FOV = pf.FOV
SEEDS = list(range(100, 164))      # the closed forms' 64 fixed seeds


@pytest.fixture(scope="module")
def path_lib():
    return tl.load()


_report = tl.reporter("path lights", "test_path_light_host")


BOX = ((0.1, -0.2, -1.5), (0.3, 0.5, 0.2), (0.2, 0.4, -0.3))
# The sampler is seen from a point on the box's body diagonal, two units from its centre: its three visible faces are seen at cosines
# of 0.4 to 0.75.  fp32 forms both pdfs through n . wl and a distance along wl, whose rounding (a few 2^-24) is divided by that
# cosine: about 1e-6 relative there, inside the 1e-5 the two pdfs have to agree to; at grazing incidence no fp32 routine could.
BOX_VIEW = np.asarray(BOX[0]) + 2.0 * pl.rotation(BOX[2]) @ (np.ones(3) / np.sqrt(3.0))


def _light_box():
    """The sampler's light: a box of unequal sides (12 triangles, three distinct areas) plus one degenerate triangle, before a
    one-triangle depth mesh -> (V, T, objects)."""
    Vb, Tb = pl.box(*BOX)
    Tb = np.concatenate([Tb[:5], [[0, 0, 3]], Tb[5:]]).astype(np.int32)     # a degenerate triangle in the middle of the list
    Vs, Ts = pp.FAR_TRIANGLE
    return Vs, Ts, [{"vertices": Vb, "triangles": Tb, "bsdf": {"type": "area", "radiance": (1.0, 2.0, 3.0)}}]


# ---- 0: the symbols ----------------------------------------------------------------------------------------------------------------------
def test_symbols(path_lib):
    with open(os.path.join(ROOT, "include", "matpbr_path.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(matpbr_path_\w+)\s*\(", text))
    new = {"matpbr_path_light_tables", "matpbr_path_render_objects_lights", "matpbr_path_light_sample_host", "matpbr_path_light_pdf_host"}
    assert new <= declared and set(path_lib.LIGHT_SYMBOLS) == new and new <= set(path_lib.LATE_SYMBOLS)
    lib = path_lib.load()
    for name in new:
        fn = path_lib.symbol(name, lib)
        assert fn.argtypes == path_lib.SIGNATURES[name][1] and fn.restype == path_lib.SIGNATURES[name][0], name
    assert lib.matpbr_path_version() == 3 == path_lib.VERSION
    assert "MATPBR_PATH_BSDF_AREA = 4" in text and path_lib.BSDF_AREA == 4
    assert ctypes.sizeof(path_lib.PathLights) == 4 + 4 * 8 * 4 and ctypes.sizeof(path_lib.PathObject) == 24

    class Old:
        pass

    for name in new:
        with pytest.raises(path_lib.PathError, match=name):
            path_lib.symbol(name, Old())


# ---- 1: the sampler on the CPU entry points ------------------------------------------------------------------------------------------------
def test_sampler_on_the_cpu_entry_points(path_lib):
    Vs, Ts, objects = _light_box()
    V, T, table, records, lt = path_lib.merge_objects(Vs, Ts, objects, pbr=True, lights=True)
    head = lt["header"]
    assert head.n_lights == 1 and head.n_tri[0] == 13 and head.first[0] == 0 and head.object[0] == 0
    P = V[T[1:]]
    area = 0.5 * np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=-1)
    assert area[5] == 0 and len(set(np.round(area[area > 0], 9))) == 3
    n = 1 << 16
    g = (np.arange(256) + 0.5) / 256
    u3, u4 = (x.reshape(-1) for x in np.meshgrid(g, g, indexing="ij"))
    u = np.stack([(np.arange(n) + 0.5) / n, u3, u4, np.zeros(n)], -1).astype(np.float32)      # u2 stratified; (u3, u4) a grid
    po_ = np.tile(BOX_VIEW.astype(np.float32), (n, 1))
    for have_env in (False, True):
        n_e = 1 + have_env
        s = path_lib.light_sample_host(lt, have_env, po_, u)
        lit = s["record"] >= 0
        assert np.array_equal(lit, s["emitter"] == n_e - 1) and abs(lit.mean() - 1 / n_e) < 1e-3
        rec = s["record"][lit]
        assert rec.min() >= 0 and rec.max() <= 12 and not (rec == 5).any()              # the degenerate triangle is never chosen
        # the points lie on the chosen triangle
        tri = lt["tris"][rec]
        v0, e1, e2 = tri[:, 0, :3].astype(np.float64), tri[:, 1, :3].astype(np.float64), tri[:, 2, :3].astype(np.float64)
        rel = s["y"][lit].astype(np.float64) - v0
        nl = np.cross(e1, e2)
        nl /= np.linalg.norm(nl, axis=-1, keepdims=True)
        assert np.abs((rel * nl).sum(-1)).max() < 1e-6
        g11, g12, g22 = (e1 * e1).sum(-1), (e1 * e2).sum(-1), (e2 * e2).sum(-1)       # barycentrics by the 2 x 2 normal equations
        r1, r2, det = (rel * e1).sum(-1), (rel * e2).sum(-1), g11 * g22 - g12 * g12
        b1, b2 = (g22 * r1 - g12 * r2) / det, (g11 * r2 - g12 * r1) / det
        assert min(b1.min(), b2.min()) > -1e-5 and (b1 + b2).max() < 1 + 1e-5
        # counts per triangle follow area to within binomial 5 sigma
        N = int(lit.sum())
        for t in range(13):
            p = area[t] / area.sum()
            assert abs((rec == t).sum() - N * p) <= 5 * np.sqrt(N * p * (1 - p)) + 1e-9, (t, (rec == t).sum(), N * p)
        # the classic MIS bug: the hit side's pdf at the sampled direction is the sampler's
        ok = lit & (s["pdf"] > 0)
        assert ok.sum() > 0.2 * N
        t, pdf = path_lib.light_pdf_host(lt, have_env, np.zeros(ok.sum(), np.int32), s["record"][ok], po_[ok], s["wl"][ok])
        assert np.abs(t / s["dist"][ok] - 1).max() < 1e-5
        worst = np.abs(pdf / s["pdf"][ok] - 1).max()
        _report(f"hit-side pdf against the sampler's, n_e = {n_e}: worst relative difference", f"{worst:.2e}")
        assert worst < 1e-5
        # and the sampler's pdf is dist^2 / (A cos n_e) in fp64
        d = s["y"][ok].astype(np.float64) - po_[ok]
        dist = np.linalg.norm(d, axis=-1)
        cos_l = -((d / dist[:, None]) * nl[ok[lit]]).sum(-1)
        assert np.abs(s["pdf"][ok] / (dist ** 2 / (area.sum() * cos_l * n_e)) - 1).max() < 1e-4
    # u2 at 0, at every idx / n_e boundary and at 1 - 2^-24 stays in range
    four = path_lib.PathLights()
    four.n_lights = 3
    tris3 = np.concatenate([lt["tris"]] * 3)
    cdf3 = np.concatenate([lt["cdf"]] * 3)
    for l in range(3):
        four.object[l], four.first[l], four.n_tri[l], four.area[l] = l, 13 * l, 13, head.area[0]
    lt3 = {"header": four, "tris": tris3, "cdf": cdf3}
    for have_env in (False, True):
        n_e = 3 + have_env
        edge = [0.0, 1 - 2.0 ** -24] + [k / n_e for k in range(1, n_e)] + [np.nextafter(np.float32(k / n_e), np.float32(0)) for k in range(1, n_e)]
        uu = np.zeros((len(edge), 4), np.float32)
        uu[:, 0], uu[:, 1:3] = edge, 0.3
        s = path_lib.light_sample_host(lt3, have_env, po_[:len(edge)], uu)
        assert s["emitter"].min() >= 0 and s["emitter"].max() == n_e - 1 and s["emitter"][0] == 0 and s["emitter"][1] == n_e - 1
        assert (s["u_re"] >= 0).all() and (s["u_re"] < 1).all()
        lit = s["record"] >= 0
        l = s["emitter"][lit] - have_env
        assert ((s["record"][lit] >= 13 * l) & (s["record"][lit] < 13 * (l + 1))).all()
        idx, u_re = pl.choose(uu[:, 0], n_e)                          # the restatement's choice is the library's
        assert np.array_equal(idx, s["emitter"]) and np.array_equal(u_re.astype(np.float32), s["u_re"])


# ---- 2: light_tables ----------------------------------------------------------------------------------------------------------------------
def test_light_tables_against_fp64_and_refusals(path_lib):
    Vs, Ts, objects = _light_box()
    Vq, Tq = pl.quad(pl.LIGHT_QUAD)
    Vc, Tc = po.cube((0.0, 0.0, -1.0), 0.1, (0.0, 0.0, 0.0))
    objects = [objects[0], {"vertices": Vc, "triangles": Tc, "bsdf": po.DIFFUSE_08}, {"vertices": Vq, "triangles": Tq, "bsdf": pl.QUAD_LIGHT}]
    V, T, table, records, lt = path_lib.merge_objects(Vs, Ts, objects, pbr=True, lights=True)
    head = lt["header"]
    assert [t.kind for t in table] == [4, 2, 4] and tuple(table[0].p) == (1.0, 2.0, 3.0) and tuple(table[2].p) == (25.0, 24.0, 20.0)
    assert head.n_lights == 2 and list(head.object)[:2] == [0, 2] and list(head.first)[:2] == [0, 13] and list(head.n_tri)[:2] == [13, 2]
    assert lt["tris"].shape == (15, 3, 4) and lt["cdf"].shape == (15,)
    for l, ob in enumerate((table[0], table[2])):
        P = V[T[ob.first_tri:ob.first_tri + ob.n_tri]]
        _, A, cdf = pl.light_table(P)
        sl = slice(head.first[l], head.first[l] + head.n_tri[l])
        assert head.area[l] == np.float32(A) and np.array_equal(lt["cdf"][sl], cdf) and lt["cdf"][sl][-1] == 1.0
        assert np.array_equal(lt["tris"][sl, 0, :3], P[:, 0].astype(np.float32))
        assert np.array_equal(lt["tris"][sl, 1, :3], (P[:, 1] - P[:, 0]).astype(np.float32))
        assert np.array_equal(lt["tris"][sl, 2, :3], (P[:, 2] - P[:, 0]).astype(np.float32)) and not lt["tris"][sl, :, 3].any()
    # a table without lights: no tables, and the wrapper's other values are what they were
    assert path_lib.merge_objects(Vs, Ts, [objects[1]], lights=True)[-1] is None
    assert len(path_lib.merge_objects(Vs, Ts, [objects[1]])) == 3
    # refusals
    lib = path_lib.load()
    P_ = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    Vd, Td = np.ascontiguousarray(V, np.float64), np.ascontiguousarray(T, np.int32)
    head2, n = path_lib.PathLights(), ctypes.c_long(0)

    def tables(kind, p, first=1, n_tri=13):
        ob = (path_lib.PathObject * 1)(path_lib.PathObject(kind, first, n_tri, (ctypes.c_float * 3)(*p)))
        return lib.matpbr_path_light_tables(P_(Vd), Vd.shape[0], P_(Td), Td.shape[0], ctypes.cast(ob, ctypes.c_void_p), 1, None,
                                            ctypes.cast(ctypes.byref(head2), ctypes.c_void_p), None, None, 0, ctypes.cast(ctypes.byref(n), ctypes.c_void_p))

    nan, inf = float("nan"), float("inf")
    assert tables(4, (1.0, 0.0, 2.0)) == 0 and n.value == 13 and head2.n_lights == 1
    assert tables(4, (0.0, 0.0, 0.0)) == 0                              # a radiance of 0 is valid
    assert tables(2, (0.5, 0.5, 0.5)) == 0 and n.value == 0 and head2.n_lights == 0
    for p in ((-1.0, 0.0, 0.0), (nan, 1.0, 1.0), (1.0, inf, 1.0), (1.0, 1.0, -0.0001)):
        assert tables(4, p) == -1, p                                    # a negative or non-finite radiance
    assert tables(0x104, (1.0, 1.0, 1.0)) == -1                         # kind 4 with the smooth flag
    assert tables(5, (1.0, 1.0, 1.0)) == -1
    assert tables(4, (1.0, 1.0, 1.0), first=6, n_tri=1) == -1           # a light of total area 0: the degenerate triangle alone
    assert tables(4, (1.0, 1.0, 1.0), first=10, n_tri=100) == -1        # a range outside the mesh
    with pytest.raises(path_lib.PathError, match="matpbr_path_light_tables"):
        path_lib.merge_objects(Vs, Ts, [{"vertices": Vq, "triangles": np.array([[0, 0, 1]], np.int32), "bsdf": pl.QUAD_LIGHT}], lights=True)
    # every other entry point refuses kind 4 as an unknown kind; the light entry point its own bad arguments (validation precedes the launch)
    one = np.zeros(4, np.float32)
    tab = lambda t: ctypes.cast(t, ctypes.c_void_p)
    obj = lambda k, p=(1.0, 1.0, 1.0): (path_lib.PathObject * 1)(path_lib.PathObject(k, 1, 13, (ctypes.c_float * 3)(*p)))
    headp = lambda h: ctypes.cast(ctypes.byref(h), ctypes.c_void_p)
    frame = [P_(one)] * 5 + [4, 4, 35.0] + [P_(one)] * 4 + [2, 4, 1, 4, 0, 1, P_(one), None, None]
    assert lib.matpbr_path_render_objects(*frame, tab(obj(4)), 1) == -1
    assert lib.matpbr_path_render_objects_normals(*frame, tab(obj(4)), 1, P_(one), 1) == -1
    assert lib.matpbr_path_render_objects_pbr(*frame, tab(obj(4)), 1, None, 1, None) == -1
    good = path_lib.PathLights()
    good.n_lights, good.object[0], good.first[0], good.n_tri[0], good.area[0] = 1, 0, 0, 13, 1.0
    aligned = np.zeros(64, np.float32)
    buf = aligned[(-aligned.ctypes.data % 16) // 4:]
    render = lib.matpbr_path_render_objects_lights
    tail = lambda o, h, t=buf, c=one: (tab(o), 1, None, 1, None, headp(h) if h is not None else None, P_(t) if t is not None else None,
                                       P_(c) if c is not None else None)
    for p in ((-1.0, 0.0, 0.0), (nan, 1.0, 1.0), (1.0, inf, 1.0)):
        assert render(*frame, *tail(obj(4, p), good)) == -1
    assert render(*frame, *tail(obj(0x104), good)) == -1
    assert render(*frame, *tail(obj(4), None)) == -1                    # null tables with a kind-4 object
    assert render(*frame, *tail(obj(4), good, None)) == -1
    assert render(*frame, *tail(obj(4), good, buf, None)) == -1
    for field, value in (("n_lights", 2), ("n_lights", 0)):
        bad = path_lib.PathLights.from_buffer_copy(good)
        setattr(bad, field, value)
        assert render(*frame, *tail(obj(4), bad)) == -1
    for field, value in (("object", 1), ("first", 1), ("n_tri", 12), ("area", 0.0), ("area", nan), ("area", -1.0)):
        bad = path_lib.PathLights.from_buffer_copy(good)
        getattr(bad, field)[0] = value
        assert render(*frame, *tail(obj(4), bad)) == -1, (field, value)
    bad_depth = list(frame)
    bad_depth[15] = 17
    assert render(*bad_depth, *tail(obj(4), good)) == -1                # a valid table, max_depth beyond the limit: still before any launch
    # the features take kind 4: id 1 + k and the face normal (host entry point)
    Vl, Tl = pp.quad()
    Vm, Tm, tb, _, _ = path_lib.merge_objects(Vs, Ts, [{"vertices": Vl, "triangles": Tl, "bsdf": {"type": "area", "radiance": 2.0}}], normals=True, pbr=True)
    geom = path_lib.features_host(path_lib.build_bvh(Vm, Tm, 1), 5, 6, FOV, tb, None, 1)
    assert np.all(geom[..., 7] == 1.0) and np.abs(geom[..., 4:7] - [0.0, 0.0, 1.0]).max() <= 1e-6
    with pytest.raises(path_lib.PathError):                             # the lookup of the PBR entry point still knows no kind 4
        path_lib.object_lookup_host(tb, None, np.array([1], np.int32))


# ---- 3: the restatement against closed forms ----------------------------------------------------------------------------------------------
def _closed_form(path_lib, objects, env, max_depth, expected, covered, label, H=10, W=12):
    Vs, Ts = pp.FAR_TRIANGLE
    V, T, table = pob.merged(Vs, Ts, objects)
    vals = pob.replay_mean(H, W, 16, SEEDS, max_depth, V, T, env, path_lib.env_tables(env), table, chunk=4)
    ok, worst = pl.within_five_sigma(vals, expected, covered)
    _report(f"{label}: worst |mean - expected| / (5 se + 1e-3 expected) over {int(covered.sum())} pixels", f"{worst:.3f}")
    assert covered.sum() >= 12 and ok, (label, worst)


def test_restatement_against_lamberts_polygon_formula(path_lib):
    """(a) A diffuse floor quad under a downward-facing emitter quad, zero envmap, max_depth 2: the pixel is rho / pi times Lambert's
    polygon irradiance averaged over its footprint (8 x 8 midpoints).  64 fixed seeds x spp 16 at 12 x 10, 5 standard errors."""
    expected, covered = pl.lambert_expected(10, 12)
    assert expected[covered].min() > 0
    _closed_form(path_lib, pl.lambert_scene(), np.zeros((4, 8, 3), np.float32), 2, expected, covered, "Lambert's polygon formula")


@pytest.mark.parametrize("inner,max_depth", [("diffuse", 2), ("glass", 16)])
@pytest.mark.parametrize("env_value", [0.0, 5.0])
def test_restatement_in_the_furnace_box(path_lib, inner, max_depth, env_value):
    """(b) A closed box that emits L inwards around the camera and a convex diffuse object (rho L at max_depth 2) or a glass sphere
    (L at max_depth 16); a bright constant envmap outside changes nothing but n_e."""
    objects = pl.furnace_scene(inner)
    inside, _ = tl.footprints(objects[1:], 10, 12)
    value = (np.asarray(pl.FURNACE_RHO) if inner == "diffuse" else np.ones(3)) * pl.f32(pl.FURNACE_L)
    expected = np.broadcast_to(value, (10, 12, 3)).copy()
    _closed_form(path_lib, objects, np.full((4, 8, 3), env_value, np.float32), max_depth, expected, inside, f"furnace, {inner}, envmap {env_value}")


# ---- 4: routing and bits on the host -------------------------------------------------------------------------------------------------------
def test_restatement_without_lights_is_the_pbr_restatement(oracle64, path_lib):
    """On the PBR table the walk returns the bits the PBR restatement returned before the walks were folded into one
    (`path_testlib.recorded_walk`)."""
    from materialist_amd import mesh

    H, W = 10, 12
    rm = mesh.reference_mesh(pf.groove_scene(H, W), FOV)
    rng = np.random.default_rng(11)
    a, r, m = pf.groove_maps(H, W, rng)
    env = pf.groove_env(rng)
    V, T, table = pob.merged(rm["vertices"], rm["triangles"], pp.table_scene())
    args = (oracle64, V, T, a, r, m, env, path_lib.env_tables(env), H, W, 6, 1, table)
    rec0 = tl.recorded_walk("pbr")
    ref = rec0["L"]
    got, rec1 = pob.replay_objects(*args)
    assert np.array_equal(ref, got) and rec1["n_e"] == 1
    assert all(np.array_equal(rec0[k], rec1[k]) for k in ("transmitted", "diffuse_object", "blocked_by_object", "fallback", "pbr_vertex"))


def test_object_bsdf_merge_objects_and_the_scene_file(path_lib, tmp_path):
    from materialist_amd import mesh, relight

    assert path_lib.object_bsdf({"type": "area", "radiance": 2.5}) == (4, (2.5, 2.5, 2.5))
    assert path_lib.object_bsdf({"type": "area", "radiance": [1, 0, 3]}) == (4, (1.0, 0.0, 3.0))
    assert path_lib.object_bsdf({"type": "area"}) == (4, (1.0, 1.0, 1.0))
    nan, inf = float("nan"), float("inf")
    for bad in (-0.5, nan, inf, [1.0, -1.0, 1.0], [1.0, 2.0], [[1.0, 2.0, 3.0]], 1e39, "bright"):
        with pytest.raises(ValueError, match="radiance"):
            path_lib.object_bsdf({"type": "area", "radiance": bad})
    assert path_lib.object_bsdf(po.GLASS) == (1, (1.49, 1.000277, 0.0)) and path_lib.object_bsdf(pp.PLASTIC)[0] == 3
    Vs, Ts = pp.FAR_TRIANGLE
    Vq, Tq = pl.quad(pl.LIGHT_QUAD)
    lamp = {"vertices": Vq, "triangles": Tq, "bsdf": pl.QUAD_LIGHT}
    with pytest.raises(ValueError, match="normals"):
        path_lib.merge_objects(Vs, Ts, [dict(lamp, normals=np.tile([0.0, 0.0, 1.0], (4, 1)))])
    V, T, table = path_lib.merge_objects(Vs, Ts, [lamp])
    assert table[0].kind == 4 and (table[0].first_tri, table[0].n_tri) == (1, 2) and tuple(table[0].p) == (25.0, 24.0, 20.0)
    # the object list file: the new type, and the error texts for a bad radiance
    os.makedirs(tmp_path / "lists")
    mesh.write_ply(str(tmp_path / "lists" / "lamp.ply"), Vq, Tq)
    path = str(tmp_path / "lists" / "lamp.json")

    def write(doc):
        with open(path, "w") as f:
            json.dump(doc, f)

    write({"objects": [{"ply": "lamp.ply", "bsdf": {"type": "area", "radiance": [30, 28, 20]}}]})
    got = relight.load_oi_scene(path)
    assert got[0]["bsdf"] == {"type": "area", "radiance": [30, 28, 20]} and got[0]["normals"] == "flat"
    for rad, pattern in ((-1.0, r"objects\[0\].*bad bsdf.*radiance must be finite and >= 0"), ([1.0, 2.0], r"objects\[0\].*bad bsdf.*radiance must be a scalar or 3 values"),
                         ("x", r"objects\[0\].*bad bsdf.*radiance")):
        write({"objects": [{"ply": "lamp.ply", "bsdf": {"type": "area", "radiance": rad}}]})
        with pytest.raises(ValueError, match=pattern) as e:
            relight.load_oi_scene(path)
        assert "lamp.json" in str(e.value)
    write({"objects": [{"ply": "lamp.ply", "bsdf": {"type": "area"}, "normals": "vertex"}]})
    with pytest.raises(ValueError, match=r"objects\[0\].*'normals' must be 'flat' for an area light"):
        relight.load_oi_scene(path)
    # the albedo guide gives 1 on a light
    import torch

    geom = torch.zeros(2, 2, 8)
    geom[..., 7] = torch.tensor([[0.0, 1.0], [2.0, -1.0]])
    guide = relight.albedo_guide(geom, torch.full((2, 2, 3), 0.25), [{"type": "area", "radiance": 9.0}, po.DIFFUSE_08]).numpy()
    assert np.all(guide[0, 1] == 1.0) and np.all(guide[0, 0] == 0.25) and np.all(guide[1, 0] == np.float32(0.8)) and np.all(guide[1, 1] == 0.0)
    # --env_scale
    import render_final

    a = render_final.parse_args(["--save_name", "case", "--mode", "oi", "--env_scale", "0"])
    assert a.env_scale == 0.0 and render_final.parse_args(["--save_name", "case", "--mode", "oi"]).env_scale == 1.0
    for argv in (["--mode", "real", "--env_scale", "2"], ["--mode", "oi", "--env_scale", "-1"], ["--mode", "oi", "--env_scale", "nan"]):
        with pytest.raises(SystemExit):
            render_final.parse_args(["--save_name", "case"] + argv)
    env = np.ones((2, 4, 3), np.float32)
    assert relight._scaled_env(env, 1.0) is env and np.all(relight._scaled_env(env, 0.0) == 0) and np.all(relight._scaled_env(env, 2.5) == 2.5)
    with pytest.raises(ValueError, match="env_scale"):
        relight._scaled_env(env, 2.0, "sh")


def test_a_table_without_lights_leaves_every_route_alone(path_lib, monkeypatch):
    """`PathTracer` without an area light calls what it called: the constructor builds no light tables and asks for no light symbol."""
    asked = []
    real = path_lib.symbol
    monkeypatch.setattr(path_lib, "symbol", lambda name, lib=None: (asked.append(name), real(name, lib))[1])
    monkeypatch.setattr(path_lib.torch, "from_numpy", lambda x: _Host(x))
    Vs, Ts = pp.FAR_TRIANGLE
    for objects, want in ((pp.table_scene(), {"matpbr_path_render_objects_pbr", "matpbr_path_render_objects_normals"}),
                          (po.two_cubes(), set()), (None, set())):
        del asked[:]
        tracer = path_lib.PathTracer(Vs, Ts, 4, 4, FOV, device="cpu", objects=objects)
        assert set(asked) == want and tracer.lights is None and tracer.stats["n_lights"] == 0
    tracer = path_lib.PathTracer(Vs, Ts, 4, 4, FOV, device="cpu", objects=pl.table_scene())
    assert tracer.stats["n_lights"] == 2 and tracer.stats["n_pbr_objects"] == 1 and tracer.lights is not None and tracer.pbr is not None
    assert "matpbr_path_render_objects_lights" in asked


class _Host:
    """torch.from_numpy's result for a tracer built without a device: keeps the array, `.to()` returns itself."""

    def __init__(self, x):
        self.x = x

    def to(self, *a, **k):
        return self


# ---- 5: the GPU test's scene ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_on", [True, False])
def test_restatement_over_fp32_and_fp64_traversal(path_lib, oracle64, env_on):
    """The GPU criterion's ground: over the library's fp32 traversal and over the fp64 brute force the restatement disagrees in NO
    pixel of the GPU test's renders (the groove at 24 x 20 with `path_light_fp64.table_scene`; max_depth 2, 6, 16; seeds 0-2; the
    envmap on, n_e = 3, and zero, n_e = 2), and every render holds every kind of light path."""
    from materialist_amd import mesh

    H, W = 20, 24
    rm = mesh.reference_mesh(pf.groove_scene(H, W), FOV)
    rng = np.random.default_rng(11)
    a, r, m = pf.groove_maps(H, W, rng)
    env = pf.groove_env(rng) if env_on else np.zeros((8, 16, 3), np.float32)
    objects = pl.table_scene()
    V, T, table = pob.merged(rm["vertices"], rm["triangles"], objects)
    Vm, Tm, tb, corner, records, lt = path_lib.merge_objects(rm["vertices"], rm["triangles"], objects, normals=True, pbr=True, lights=True)
    n_scene = rm["triangles"].shape[0]
    assert [t.kind for t in tb] == [4, 4, 0x101, 3, 2] and lt["header"].n_lights == 2
    bvh = path_lib.build_bvh(Vm, Tm, n_scene)

    def closest(o, d):
        t, k = path_lib.trace_host(bvh, o, d)
        return np.where(k < 0, np.inf, t.astype(np.float64)), k.astype(np.int64)

    tab = path_lib.env_tables(env)
    seen = {k: 0 for k in pl.RECORD_KEYS}
    for max_depth in (2, 6, 16):
        for seed in (0, 1, 2):
            args = (oracle64, V, T, a, r, m, env, tab, H, W, max_depth, seed, table)
            L64, rec = pob.replay_objects(*args)
            L32, _ = pob.replay_objects(*args, closest=closest)
            assert rec["n_e"] == 2 + env_on
            err = (np.abs(L32 - L64) / np.maximum(np.abs(L64), np.abs(L64).mean())).max(-1)
            assert int((err > 1e-3).sum()) == 0, (max_depth, seed, np.argwhere(err > 1e-3)[:10])
            for k in pl.RECORD_KEYS:
                # every kind of light path, in every one of the renders.  A light behind glass needs three segments (camera to
                # glass, through it, on to the light): max_depth 2 traces two, and only a mirror reflection off the glass could
                # show a light there, which no lane of these seeds draws
                assert rec[k].any() or (k == "light_through_glass" and max_depth == 2), (k, max_depth, seed)
                seen[k] += int(rec[k].sum())
    _report(f"envmap {'on' if env_on else 'zero'}: pixels with " + " / ".join(pl.RECORD_KEYS) + " (9 renders)", " / ".join(str(seen[k]) for k in pl.RECORD_KEYS))
