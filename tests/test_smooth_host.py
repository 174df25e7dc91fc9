"""Mesh adjacency, smoothing and vertex normals without a GPU: the header, the binding, the constants and every refusal of the five entries (they come before any
device call), and the definition (tests/smooth_ref.py, the numpy restatement the GPU tests compare with bit for bit) pinned on subdivided spheres: closed surfaces
of Euler characteristic 2, the hemisphere's boundary, what Taubin's filter and the plain Laplacian do to a noisy sphere, the three boundary modes, invariance under
a permutation of the faces, and normals that point along the radius."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np

import smooth_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INVALID_ARG, WORKSPACE = 1, 4
NAMES = ["nrf_mesh_adjacency_workspace_bytes", "nrf_mesh_adjacency_count", "nrf_mesh_adjacency_emit", "nrf_mesh_smooth", "nrf_mesh_vertex_normals"]


@functools.lru_cache(maxsize=None)
def closed(level):
    verts, faces = S.sphere(level)
    return verts, faces, S.adjacency(faces, len(verts))


@functools.lru_cache(maxsize=None)
def half(level=3):
    verts, faces = S.hemisphere(level)
    return verts, faces, S.adjacency(faces, len(verts))


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def radius(p):
    return np.linalg.norm(np.asarray(p, np.float64) - np.asarray(S.CENTRE), axis=1)


def test_header_binding_and_constants_agree():
    from nerfpp_amd import _lib, mesh
    hdr = open(os.path.join(ROOT, "include", "nerfpp_hip.h")).read()
    for name, value in (("ADJ_BOUNDARY", 1), ("ADJ_NONMANIFOLD", 2), ("ADJ_SHORT_ROW", 32), ("SMOOTH_MAX_CHANNELS", 4), ("SMOOTH_FREE", 0), ("SMOOTH_FIXED", 1),
                        ("SMOOTH_CURVE", 2), ("NORMALS_AREA", 0), ("NORMALS_UNIT", 1)):
        m = re.search(rf"#define\s+NRF_{name}\s+(\d+)", hdr)
        assert m and int(m[1]) == value == getattr(mesh, name) == getattr(S, name), name
    want = dict(zip(NAMES, (("z", "ll"), ("i", "pllpppzp"), ("i", "pllllppppppppzp"), ("i", "pppliiffipppplp"), ("i", "plplpplipp"))))
    at = _lib.SYMBOLS.index("nrf_texture_shade")
    assert _lib.SYMBOLS[at + 1:at + 7] == NAMES + ["nrf_density_grad_workspace_bytes"], "directly after nrf_texture_shade, in the header's order"
    section = hdr.index("Mesh adjacency, smoothing and vertex normals")
    assert hdr.index("nrf_texture_shade(") < section < hdr.index("nrf_mesh_adjacency_workspace_bytes(") < hdr.index("Density gradient")
    text = hdr[section:hdr.index("Density gradient")]
    assert "NRF_ADJ_SHORT_ROW" in text and "NOT invariant under a permutation of the faces" in text, "the header states the row threshold and the order dependence"
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig and hasattr(lib, name) and re.search(rf"NRF_API (size_t|int) {name}\(", hdr), name
    for name in ("BuildAdjacency", "MeshTopology", "VertexNormals", "SmoothMesh", "SmoothAttributes", "MeshAdjacency"):
        assert callable(getattr(mesh, name)), name
    params = inspect.signature(mesh.ExtractMesh).parameters
    assert params["smooth_iterations"].default == 0
    sm = inspect.signature(mesh.SmoothMesh).parameters
    assert [(k, sm[k].default) for k in list(sm)[1:]] == [("iterations", 10), ("lam", 0.5), ("mu", -0.53), ("boundary", "curve"), ("attributes", ()),
                                                           ("recompute_normals", True), ("adjacency", None)]
    sa = inspect.signature(mesh.SmoothAttributes).parameters
    assert (sa["lam"].default, sa["mu"].default, sa["boundary"].default) == (0.5, 0.0, "free") and sa["iterations"].default is inspect.Parameter.empty


def test_workspace_sizes_and_refusals_need_no_gpu():
    """Every bad argument of the header is refused before anything touches the device, so the whole list is checked here over pointers that are never dereferenced."""
    from nerfpp_amd import _lib
    lib = _lib.lib()
    fake, fake2, fake3 = C.c_void_p(256), C.c_void_p(1 << 20), C.c_void_p(1 << 21)
    big = 1 << 40
    nan, inf = float("nan"), float("inf")

    def refused(name, status, fn, cases):
        for kw in cases:
            assert fn(**kw) == status, (name, kw)
            assert lib.nrf_last_error().startswith(name.encode()), (kw, lib.nrf_last_error())

    size = lib.nrf_mesh_adjacency_workspace_bytes
    # per vertex four int32 and two int64 starts, per face 18 int32 (two copies of its 3 row entries and of its 6 half-edge ends)
    assert size(258, 512) >= 258 * 32 + 512 * 72 and size(0, 0) > 0 and size(258, 513) > size(258, 512) and size(2 ** 31 - 1, 2 ** 31 - 1) > 2 ** 37
    for bad in ((-1, 1), (1, -1), (2 ** 31, 1), (1, 2 ** 31)):
        assert size(*bad) == 0, bad

    shapes = [dict(nv=-1), dict(nv=2 ** 31), dict(nf=-1), dict(nf=2 ** 31), dict(faces=None), dict(ws=None), dict(ws=C.c_void_p(260))]

    def count(faces=fake, nv=4, nf=2, n_i=fake, n_n=fake, ws=fake, ws_bytes=big):
        return lib.nrf_mesh_adjacency_count(faces, nv, nf, n_i, n_n, ws, ws_bytes, None)

    refused("nrf_mesh_adjacency_count", INVALID_ARG, count, shapes + [dict(n_i=None), dict(n_n=None)])
    refused("nrf_mesh_adjacency_count", WORKSPACE, count, [dict(ws_bytes=size(4, 2) - 1), dict(ws_bytes=0)])

    def emit(faces=fake, nv=4, nf=2, ni=6, nn=10, fs=fake, fl=fake, ns=fake, nb=fake, nbf=fake, flags=fake, stats=fake, ws=fake, ws_bytes=big):
        return lib.nrf_mesh_adjacency_emit(faces, nv, nf, ni, nn, fs, fl, ns, nb, nbf, flags, stats, ws, ws_bytes, None)

    refused("nrf_mesh_adjacency_emit", INVALID_ARG, emit, shapes + [dict(ni=-1), dict(nn=-1), dict(ni=7), dict(nn=13), dict(fs=None), dict(fl=None), dict(ns=None),
                                                                    dict(nb=None), dict(nbf=None), dict(flags=None), dict(stats=None)])
    refused("nrf_mesh_adjacency_emit", WORKSPACE, emit, [dict(ws_bytes=size(4, 2) - 1), dict(ws_bytes=0)])

    def smooth(x=fake, out=fake2, tmp=fake3, nv=4, c=3, it=1, lam=0.5, mu=-0.53, mode=S.SMOOTH_CURVE, ns=fake, nb=fake, nbf=fake, flags=fake, nn=10):
        return lib.nrf_mesh_smooth(x, out, tmp, nv, c, it, lam, mu, mode, ns, nb, nbf, flags, nn, None)

    refused("nrf_mesh_smooth", INVALID_ARG, smooth, [
        dict(nv=-1), dict(nv=2 ** 31), dict(nn=-1), dict(c=0), dict(c=5), dict(c=-1), dict(it=-1), dict(mode=-1), dict(mode=3), dict(lam=nan), dict(lam=inf),
        dict(lam=-inf), dict(mu=nan), dict(mu=inf), dict(mu=-inf), dict(x=None), dict(out=None), dict(tmp=None), dict(ns=None), dict(nb=None), dict(nbf=None),
        dict(flags=None), dict(flags=None, mode=S.SMOOTH_FIXED), dict(out=fake), dict(tmp=fake), dict(tmp=fake2), dict(x=fake2), dict(x=C.c_void_p(258)),
        dict(c=2, out=C.c_void_p(260)), dict(c=4, tmp=C.c_void_p(264)), dict(it=2 ** 30)])

    def normals(verts=fake, nv=4, faces=fake2, nf=2, fs=fake, fl=fake, ni=6, w=S.NORMALS_AREA, out=fake3):
        return lib.nrf_mesh_vertex_normals(verts, nv, faces, nf, fs, fl, ni, w, out, None)

    refused("nrf_mesh_vertex_normals", INVALID_ARG, normals, [dict(nv=-1), dict(nv=2 ** 31), dict(nf=-1), dict(nf=2 ** 31), dict(ni=-1), dict(ni=7), dict(w=-1), dict(w=2),
                                                              dict(verts=None), dict(faces=None), dict(fs=None), dict(fl=None), dict(out=None), dict(out=fake)])


def test_spheres_are_closed_surfaces_of_euler_characteristic_two():
    for level in (3, 4):
        verts, faces, adj = closed(level)
        top = S.topology(adj)
        assert top["closed"] and top["manifold"] and top["euler"] == 2 and top["vertices_used"] == len(verts) and top["faces_valid"] == len(faces), top
        assert (adj["nbr_faces"] == 2).all() and (adj["flags"] == 0).all()
        assert np.diff(adj["face_start"]).max() == 6 == np.diff(adj["nbr_start"]).max() and adj["stats"].tolist()[6:] == [6, 6]
        assert len(adj["face_list"]) == 3 * len(faces) and len(adj["nbr"]) == 2 * top["edges"]
        for v in (0, 5, len(verts) - 1):          # rows ascend, and hold what a direct search finds
            row = adj["face_list"][adj["face_start"][v]:adj["face_start"][v + 1]]
            assert row.tolist() == np.nonzero((faces == v).any(axis=1))[0].tolist()
            nb = adj["nbr"][adj["nbr_start"][v]:adj["nbr_start"][v + 1]]
            assert nb.tolist() == sorted(set(faces[row].reshape(-1).tolist()) - {v})


def test_the_hemisphere_has_a_boundary_of_32_vertices():
    verts, faces, adj = half()
    top = S.topology(adj)
    assert len(faces) == 256 and int(((adj["flags"] & S.ADJ_BOUNDARY) != 0).sum()) == 32 and top["boundary_edges"] == 32 and not top["closed"] and top["manifold"]
    assert top["euler"] == 1 and top["vertices_used"] == 145 < len(verts), "a disc; the lower vertices are unused"
    unused = np.diff(adj["face_start"]) == 0
    assert (adj["flags"][unused] == 0).all() and (np.diff(adj["nbr_start"])[unused] == 0).all()


def noisy_sphere():
    verts, _, adj = closed(4)
    c = np.asarray(S.CENTRE)
    d = verts.astype(np.float64) - c
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    noise = np.random.default_rng(7).standard_normal((len(verts), 1))
    return (c + d * (S.RADIUS * (1.0 + 0.02 * noise))).astype(F32), adj


def test_taubin_removes_noise_without_shrinking_and_the_laplacian_shrinks():
    x, adj = noisy_sphere()
    r0 = radius(x)
    taubin = radius(S.smooth(x, adj, 10, 0.5, -0.53, S.SMOOTH_FREE))
    laplace = radius(S.smooth(x, adj, 10, 0.5, 0.0, S.SMOOTH_FREE))
    print(f"radius std {r0.std():.4f} -> {taubin.std():.4f}; mean radius: Taubin {taubin.mean() / r0.mean() - 1:+.2%}, Laplacian {laplace.mean() / r0.mean() - 1:+.2%}")
    assert taubin.std() <= 0.5 * r0.std()
    assert abs(taubin.mean() / r0.mean() - 1) < 0.005
    assert laplace.mean() / r0.mean() - 1 < -0.03
    # a closed surface has no boundary: the three modes are one
    want = bits(S.smooth(x, adj, 2, 0.5, -0.53, S.SMOOTH_FREE))
    for mode in (S.SMOOTH_FIXED, S.SMOOTH_CURVE):
        assert np.array_equal(bits(S.smooth(x, adj, 2, 0.5, -0.53, mode)), want)
    assert np.array_equal(bits(S.smooth(x, adj, 0, 0.5, -0.53, S.SMOOTH_FREE)), bits(x))


def test_boundary_modes_on_the_hemisphere():
    verts, _, adj = half()
    rim = (adj["flags"] & S.ADJ_BOUNDARY) != 0
    unused = np.diff(adj["face_start"]) == 0
    out = {mode: S.smooth(verts, adj, 10, 0.5, -0.53, mode) for mode in (S.SMOOTH_FREE, S.SMOOTH_FIXED, S.SMOOTH_CURVE)}
    for mode, y in out.items():
        assert np.array_equal(bits(y[unused]), bits(verts[unused])), mode
        assert (y[~unused & ~rim] != verts[~unused & ~rim]).any(), mode
    assert np.array_equal(bits(out[S.SMOOTH_FIXED][rim]), bits(verts[rim]))
    assert np.array_equal(bits(out[S.SMOOTH_CURVE][rim, 2]), bits(verts[rim, 2])), "the boundary stays in its plane"
    assert (out[S.SMOOTH_CURVE][rim, :2] != verts[rim, :2]).any(), "and moves within it"
    assert np.abs(out[S.SMOOTH_FREE][rim, 2] - verts[rim, 2]).max() > 1e-2


def test_the_order_and_winding_of_the_faces_do_not_matter():
    for verts, faces, adj in (closed(3), half(), (*S.dirty(), S.adjacency(S.dirty()[1], 10))):
        x = np.nan_to_num(verts, nan=0.25)
        want = {mode: S.smooth(x, adj, 3, 0.5, -0.53, mode) for mode in (S.SMOOTH_FREE, S.SMOOTH_FIXED, S.SMOOTH_CURVE)}
        for seed in (1, 2):
            other = S.adjacency(S.permuted(faces, seed), len(verts))
            for k in ("face_start", "nbr_start", "nbr", "nbr_faces", "flags", "stats"):
                assert np.array_equal(other[k], adj[k]), k
            for mode, y in want.items():
                assert np.array_equal(bits(S.smooth(x, other, 3, 0.5, -0.53, mode)), bits(y)), mode


def test_the_dirty_mesh_is_counted_as_the_header_says():
    verts, faces = S.dirty()
    adj = S.adjacency(faces, len(verts))
    assert adj["stats"].tolist() == [3, 3, 9, 15, 8, 2, 5, 6] and adj["valid"].tolist() == [True] * 7 + [False] * 6 + [True]
    row = lambda v: list(zip(adj["nbr"][adj["nbr_start"][v]:adj["nbr_start"][v + 1]].tolist(), adj["nbr_faces"][adj["nbr_start"][v]:adj["nbr_start"][v + 1]].tolist()))
    assert row(0) == [(1, 3), (2, 1), (3, 1), (4, 1)] and row(7) == [(5, 2), (6, 2)] and row(9) == []
    assert adj["flags"].tolist() == [3, 3, 1, 1, 1, 3, 3, 0, 1, 0], "(5, 6) carries the duplicated face and a third one"
    y = S.smooth(verts, adj, 1, 0.5, 0.0, S.SMOOTH_FREE)
    assert np.isnan(y).any(axis=1).tolist() == [False, True, True, False, False, True, True, True, True, False], "the NaN of vertex 5 reaches its neighbours only"


def test_vertex_normals_of_the_sphere_are_radial():
    verts, faces, adj = closed(4)
    d = verts.astype(np.float64) - np.asarray(S.CENTRE)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for weighting in (S.NORMALS_AREA, S.NORMALS_UNIT):
        n = S.vertex_normals(verts, faces, adj, weighting).astype(np.float64)
        assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-6
        angle = np.degrees(np.arccos(np.clip((n * d).sum(axis=1), -1, 1)))
        print(f"weighting {weighting}: at most {angle.max():.3f} degrees from the radius")
        assert angle.max() < 2.0
    hv, hf, hadj = half()
    n = S.vertex_normals(hv, hf, hadj)
    assert (n[np.diff(hadj["face_start"]) == 0] == 0).all() and (n[np.diff(hadj["face_start"]) > 0, 2] > 0).all()
