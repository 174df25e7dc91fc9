"""Texture atlases on the MI355X: nrf_atlas_texels, nrf_texture_sample and nrf_texture_shade against the numpy restatement (tests/texture_ref.py) bit for bit, the
isolation of a face's texels from its neighbours', and the Python layer built on them: BakeTexture from a network, a TSDF volume and a callable, RenderMeshTextured,
EvaluateMesh(texture=...), and the point of it all: a textured render of a coarse mesh is closer to the colour field than its vertex-colour render."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import raster_ref as R
import texture_ref as X
import tsdf_ref as T

pytestmark = pytest.mark.gpu

F32 = np.float32
TILES = [4, 5, 8, 17]
K_SPHERE = np.array([[70.0, 0, 29.3], [0, 62.5, 22.6], [0, 0, 1]], F32)          # the camera of test_raster_gpu: fx != fy, principal point off-centre
SHADE_H, SHADE_W = 46, 58


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "needs the MI355X"
    from nerfpp_amd import _lib as L, mesh, scene, texture
    return L, texture, mesh, scene


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, F32).view(np.uint32)


def dev(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def sphere(levels):
    s = T.SPHERE
    verts, faces = R.octa_sphere(s["centre"], s["radius"], levels)
    c = np.asarray(s["centre"], F32)
    normals = ((verts - c) / np.linalg.norm(verts - c, axis=1, keepdims=True)).astype(F32)
    return verts, faces, normals


@functools.lru_cache(maxsize=None)
def mesh_case(name):
    """-> (verts, faces, normals).  s8 / s32 / s128: the octahedron subdivided 0, 1, 2 times; s7 / s31 / s127: the same without the last face, so F is odd; f0, f1;
    bad: two faces with an index out of range; degenerate: a repeated index, three vertices on a line and a face with a NaN vertex; flat: the three vertex normals of
    one face are zero (the face normal takes over) and those of another cancel half-way along an edge."""
    if name[0] == "s":
        n = int(name[1:])
        verts, faces, normals = sphere({8: 0, 32: 1, 128: 2}[n + n % 2])
        return verts, faces[:n], normals
    verts, faces, normals = sphere(1)
    faces, verts, normals = faces.copy(), verts.copy(), normals.copy()
    if name == "f0":
        return verts, faces[:0], normals
    if name == "f1":
        return verts, faces[:1], normals
    if name == "bad":
        faces[5, 1] = len(verts)
        faces[6, 2] = -1
        faces[31, 0] = 2 ** 31 - 1
    elif name == "degenerate":
        faces[3] = (faces[3, 0], faces[3, 0], faces[3, 1])
        verts = np.concatenate([verts, np.array([[0.5, 0.5, 0.5], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [np.nan, 0.0, 0.0]], F32)])
        normals = np.concatenate([normals, np.tile(np.array([[0.0, 0.0, 1.0]], F32), (4, 1))])
        faces[4] = (len(verts) - 4, len(verts) - 3, len(verts) - 2)
        faces[9, 2] = len(verts) - 1
    else:
        assert name == "flat"
        normals[faces[2]] = 0.0
        a, b = faces[20, 0], faces[20, 1]
        normals[faces[20]] = 0.0
        normals[a], normals[b] = (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)          # cancel at b0 == b1 with b2 == 0; faces that share a or b see odd normals, which is fine
    return verts, faces, normals


MESHES = ["s8", "s32", "s128", "s7", "s31", "s127", "f0", "f1", "bad", "degenerate", "flat"]


def run_texels(api, verts, faces, normals, tile, offset, slab, skip=()):
    """The C entry over row slabs of `slab` rows (None: one call) -> dict of numpy arrays; outputs named in skip are passed as NULL"""
    lib = api[0].lib()
    w, h, _, _ = X.layout(len(faces), tile)
    dv, df = dev(verts).reshape(-1, 3), dev(faces, np.int32).reshape(-1, 3)
    dn = None if normals is None else dev(normals)
    face = torch.full((h, w), -7, dtype=torch.int32, device="cuda")
    out = dict(bary=torch.full((h, w, 3), -7.0, device="cuda"), pos=torch.full((h, w, 3), -7.0, device="cuda"), rays=torch.full((h, w, 11), -7.0, device="cuda"))
    p = lambda t: None if t is None else t.data_ptr()
    step = max(h, 1) if slab is None else slab
    for r0 in range(0, max(h, 1), step):
        n = min(step, h - r0)
        at = lambda name, k: None if name in skip else out[name].data_ptr() + r0 * w * k * 4
        status = lib.nrf_atlas_texels(p(dv), len(dv), p(df), len(df), p(dn), tile, offset, r0, n, face.data_ptr() + r0 * w * 4, at("bary", 3), at("pos", 3), at("rays", 11),
                                      None)
        assert status == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    return dict(face=face.cpu().numpy(), **{k: (None if k in skip else v.cpu().numpy()) for k, v in out.items()})


# ------------------------------------------------------------------------------------ 1. nrf_atlas_texels
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name", MESHES)
def test_atlas_texels_equal_the_restatement_bit_for_bit(api, name, tile):
    verts, faces, normals = mesh_case(name)
    for nm, offset in ((normals, 0.03125), (None, 0.07), (normals, 0.0)):
        want = X.texels(verts, faces, nm, tile, offset)
        owned = want["face"] >= 0
        if name[0] == "s":
            lower, upper = (len(faces) + 1) // 2, len(faces) // 2
            assert owned.sum() == lower * tile * (tile - 1) // 2 + upper * tile * (tile + 1) // 2
        elif name in ("bad", "degenerate"):
            assert len(np.unique(want["face"][owned])) == 29 and not np.isin(want["face"], {"bad": [5, 6, 31], "degenerate": [3, 4, 9]}[name]).any()
        for slab in ((None,) if nm is None or offset == 0.0 else (None, 1, 3)):
            got = run_texels(api, verts, faces, nm, tile, offset, slab)
            assert np.array_equal(got["face"], want["face"]), (name, tile, slab, "face")
            for k in ("bary", "pos", "rays"):
                assert np.array_equal(bits(got[k]), bits(want[k])), (name, tile, slab, nm is None, k)
    if name == "flat":
        with_n, without = X.texels(verts, faces, normals, tile, 0.0), X.texels(verts, faces, None, tile, 0.0)
        f2 = with_n["face"] == 2
        assert f2.any() and np.array_equal(with_n["rays"][f2], without["rays"][f2]), "zero vertex normals: the face normal"
    got = run_texels(api, verts, faces, normals, tile, 0.03125, None, skip=("bary", "pos", "rays"))
    assert np.array_equal(got["face"], X.texels(verts, faces, normals, tile, 0.03125)["face"]), "the three float outputs may be NULL"


# ------------------------------------------------------------------------------------ 2. nrf_texture_sample
def sample_points(n_faces, seed):
    """(face [p], bary [p, 3]): corners, edge midpoints, random points of the face, barycentrics that sum to 1 +- 2^-20, points outside the face (clamped; the nearest
    filter's fallback), a NaN, an infinity, face -1 and face == F"""
    rng = np.random.default_rng(seed)
    eye = np.eye(3)
    fixed = np.concatenate([eye, (eye + np.roll(eye, 1, 0)) / 2, np.full((1, 3), 1 / 3)])
    u = np.sort(rng.uniform(0, 1, (4000, 2)), axis=1)
    rand = np.stack([u[:, 0], u[:, 1] - u[:, 0], 1 - u[:, 1]], -1)
    off = rand[:400] * (1 + 2.0 ** -20), rand[400:800] * (1 - 2.0 ** -20)
    outside = rng.uniform(-0.6, 1.6, (600, 3))
    odd = np.array([[np.nan, 0.2, 0.3], [0.2, np.nan, 0.3], [0.1, 0.3, np.nan], [0.5, np.inf, 0.1], [0.5, 0.1, -np.inf], [np.nan, np.nan, np.nan]])
    bary = np.concatenate([np.tile(fixed, (max(n_faces, 1), 1)), rand, *off, outside, odd, rand[:8]]).astype(F32)
    face = rng.integers(0, max(n_faces, 1), len(bary))
    face[:len(fixed) * max(n_faces, 1)] = np.repeat(np.arange(max(n_faces, 1)), len(fixed))          # every face at its corners and edge midpoints
    face[-8:] = [-1, n_faces, -5, n_faces + 1, 2 ** 31 - 1, -2 ** 31, n_faces, -1]
    return face.astype(np.int32), bary


def run_sample(api, tex, n_faces, tile, face, bary, flt):
    lib = api[0].lib()
    dt, dface, db = dev(tex), dev(face, np.int32), dev(bary)
    out = torch.full((len(face), tex.shape[2]), -7.0, device="cuda")
    status = lib.nrf_texture_sample(dt.data_ptr() if dt.numel() else None, n_faces, tile, tex.shape[2], dface.data_ptr(), db.data_ptr(), len(face), flt, out.data_ptr(), None)
    assert status == 0, lib.nrf_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("channels", [1, 3, 8])
@pytest.mark.parametrize("tile", TILES)
def test_texture_sample_equals_the_restatement_bit_for_bit(api, tile, channels):
    for n_faces in (128, 7, 1, 0):
        w, h, _, _ = X.layout(n_faces, tile)
        tex = np.random.default_rng(tile * 10 + channels).uniform(-1.0, 1.0, (h, w, channels)).astype(F32)
        face, bary = sample_points(n_faces, seed=n_faces + tile)
        for flt in (X.NEAREST, X.BILINEAR):
            want = X.sample(tex, n_faces, tile, face, bary, flt)
            got = run_sample(api, tex, n_faces, tile, face, bary, flt)
            assert np.array_equal(bits(got), bits(want)), (n_faces, tile, channels, flt, np.nonzero((bits(got) != bits(want)).any(-1))[0][:5])
            assert (got[-8:] == 0).all(), "face -1 and face >= F give 0"
            if n_faces:
                assert np.abs(want[:-8]).max() > 0.5
    # a texel centre gives the texel back under either filter
    n_faces, n = 7, tile - 3
    face_map, i, j = X.owners(n_faces, tile)
    tex = np.random.default_rng(1).uniform(0.0, 1.0, face_map.shape + (channels,)).astype(F32)
    inside = (face_map >= 0) & (i + j <= n)
    f, bi, bj = face_map[inside], i[inside], j[inside]
    bary = np.stack([(n - bi - bj) / n, bi / n, bj / n], -1).astype(F32)
    for flt in (X.NEAREST, X.BILINEAR):
        assert np.array_equal(run_sample(api, tex, n_faces, tile, f, bary, flt), tex[inside]), flt


# ------------------------------------------------------------------------------------ 3. isolation
@pytest.mark.parametrize("tile", TILES)
def test_bilinear_sampling_never_reads_a_texel_the_face_does_not_own(api, tile):
    """Every texel a face does not own holds NaN, and the face is sampled densely, edges and corners included: one fetch outside the face, even at weight zero,
    would make a result NaN.  Faces 0 and 1 share a cell, face 6 is the last of an odd count (the other half of its cell has no owner)."""
    n_faces, n = 7, tile - 3
    owner, _, _ = X.owners(n_faces, tile)
    rng = np.random.default_rng(tile)
    for f in (0, 1, 6):
        tex = np.where((owner == f)[..., None], rng.uniform(0.0, 1.0, owner.shape + (3,)), np.nan).astype(F32)
        parts = []
        for m in (n, 2 * n, 64, 7 * n + 1):
            a, b = np.mgrid[0:m + 1, 0:m + 1]
            keep = a + b <= m
            parts.append(np.stack([(m - a[keep] - b[keep]) / m, a[keep] / m, b[keep] / m], -1))
        u = np.sort(rng.uniform(0, 1, (3000, 2)), axis=1)
        parts.append(np.stack([u[:, 0], u[:, 1] - u[:, 0], 1 - u[:, 1]], -1))
        bary = np.concatenate(parts).astype(F32)
        face = np.full(len(bary), f, np.int32)
        got = run_sample(api, tex, n_faces, tile, face, bary, X.BILINEAR)
        assert np.isfinite(got).all(), (tile, f, int((~np.isfinite(got)).any(-1).sum()))
        assert np.array_equal(bits(got), bits(X.sample(tex, n_faces, tile, face, bary, X.BILINEAR)))
        assert np.isfinite(run_sample(api, tex, n_faces, tile, face, bary, X.NEAREST)).all()


# ------------------------------------------------------------------------------------ 4. nrf_texture_shade
@functools.lru_cache(maxsize=None)
def shade_scene():
    """The 128-face sphere and, behind it, one triangle that fills most of the image (the rasteriser's wide kernel; F = 129 is odd), rasterised by the restatement
    from two cameras at 58 x 46: the camera of test_raster_gpu and view 0 of the sphere views of test_raster_host."""
    from nerfpp_amd import scene
    verts, faces, normals = sphere(2)
    cams = [(K_SPHERE, scene.pose_spherical(67.0, -35.0, 4.0)), (scene.lego_K(SHADE_H, SHADE_W), T.sphere_views(scene.pose_spherical, scene.lego_K)[0]["c2w"])]
    views = []
    for K, c2w in cams:
        c2w = np.asarray(c2w, F32)[:3, :4]
        back = [c2w[:, 3] + c2w[:, :3] @ np.array([x, y, -6.0], F32) for x, y in ((-3.5, -2.0), (3.5, -2.0), (0.0, 3.0))]          # 6 units down the camera's -z
        v2 = np.concatenate([verts, np.array(back, F32)])
        f2 = np.concatenate([faces, np.array([[len(verts), len(verts) + 1, len(verts) + 2]], np.int32)])
        ras = R.rasterize(v2, f2, None, SHADE_H, SHADE_W, K, c2w)
        assert R.bbox_pixels(v2, f2, SHADE_H, SHADE_W, K, c2w).max() > 256 and (ras["face"] == 128).sum() > 500 and ((ras["face"] >= 0) & (ras["face"] < 128)).sum() > 150
        assert (ras["face"] < 0).sum() > 20, "some pixels see nothing"
        views.append(dict(verts=v2, faces=f2, K=K, c2w=c2w, ras=ras))
    return views


@pytest.mark.parametrize("channels", [3, 1, 8])
@pytest.mark.parametrize("tile", TILES)
def test_texture_shade_equals_the_restatement_bit_for_bit(api, tile, channels):
    L, texture, mesh, _ = api
    lib = L.lib()
    for view in shade_scene():
        verts, faces, K, c2w, ras = view["verts"], view["faces"], view["K"], view["c2w"], view["ras"]
        w, h, _, _ = X.layout(len(faces), tile)
        tex = np.random.default_rng(tile + channels).uniform(0.0, 1.0, (h, w, channels)).astype(F32)
        m = mesh.Mesh(dev(verts), dev(faces, np.int32), None)
        atlas = texture.TextureAtlas(dev(tex), tile, len(faces))
        for flt, name in ((X.BILINEAR, "bilinear"), (X.NEAREST, "nearest")):
            want = X.shade(verts, faces, ras["face"], ras["bary"], c2w, tex, tile, flt)
            assert (want[ras["face"] < 0] == 0).all() and want[ras["face"] >= 0].max() > 0.5
            # the C entry on the restatement's maps
            dv, df, dfm, dbm, dt = dev(verts), dev(faces, np.int32), dev(ras["face"], np.int32), dev(ras["bary"]), dev(tex)
            out = torch.full((SHADE_H, SHADE_W, channels), -7.0, device="cuda")
            k9, m12 = np.ascontiguousarray(K, F32).reshape(9), np.ascontiguousarray(c2w, F32).reshape(12)
            status = lib.nrf_texture_shade(dv.data_ptr(), len(dv), df.data_ptr(), len(df), dfm.data_ptr(), dbm.data_ptr(), SHADE_H, SHADE_W, k9.ctypes.data_as(C.c_void_p),
                                           m12.ctypes.data_as(C.c_void_p), dt.data_ptr(), tile, channels, flt, out.data_ptr(), None)
            assert status == 0, lib.nrf_last_error()
            torch.cuda.synchronize()
            assert np.array_equal(bits(out), bits(want)), (tile, channels, name)
            # the Python layer: the device's own rasteriser in front
            got = texture.RenderMeshTextured(m, atlas, c2w, SHADE_W, SHADE_H, K, filter=name)
            assert np.array_equal(got.FaceMap.cpu().numpy(), ras["face"]) and np.array_equal(bits(got.BaryMap), bits(ras["bary"]))
            assert np.array_equal(bits(got.DepthMap), bits(ras["depth"])) and np.array_equal(bits(got.RGBMap), bits(want)), (tile, channels, name)
            # SampleTexture at the surface barycentrics is the same device function
            valid, beta = X.surface_bary(verts, faces, ras["face"], ras["bary"], c2w)
            again = texture.SampleTexture(atlas, dev(np.where(valid, ras["face"], -1), np.int32), dev(beta), filter=name)
            assert again.shape == (SHADE_H, SHADE_W, channels) and np.array_equal(bits(again), bits(want))
    with pytest.raises(L.NrfError, match="one face order"):
        texture.RenderMeshTextured(mesh.Mesh(m.Vertices, m.Faces[:-1], None), atlas, c2w, SHADE_W, SHADE_H, K)
    with pytest.raises(L.NrfError, match="filter"):
        texture.RenderMeshTextured(m, atlas, c2w, SHADE_W, SHADE_H, K, filter="trilinear")


# ------------------------------------------------------------------------------------ 5. baking from the field
def test_bake_texture_from_a_network_and_a_tsdf_volume(api):
    """The 24^3 hash scene of the raster and TSDF tests: ExtractMesh -> SimplifyMesh -> BakeTexture.  Every source is the same call made here on the restatement's
    positions, directions and rays; EvaluateMesh(texture=) is the four scores composed by hand."""
    L, texture, mesh, scene = api
    from nerfpp_amd import metrics, raster, renderer as RR, tsdf
    sc = scene.make_hash_scene(mode="ngp", log2_t=14)
    r = sc["renderer"]
    sigma = mesh.DensityGrid(r, None, 33)
    thr = float(sigma.reshape(-1).quantile(0.7).item())
    small = mesh.SimplifyMesh(mesh.ExtractMesh(r, thr, resolution=33), resolution=10)
    nf = int(small.Faces.shape[0])
    print("faces", nf)
    assert 0 < nf < 20000
    tile = 8
    verts, faces, normals = small.Vertices.cpu().numpy(), small.Faces.cpu().numpy(), small.Normals.cpu().numpy()
    offset = 0.05
    ref = X.texels(verts, faces, normals, tile, offset)
    h, w = ref["face"].shape
    owned = dev(ref["face"] >= 0, np.bool_)
    face, bary, pos, rays = texture.AtlasTexels(small, tile, offset)
    assert np.array_equal(face.cpu().numpy(), ref["face"]) and all(np.array_equal(bits(a), bits(ref[k])) for a, k in ((bary, "bary"), (pos, "pos"), (rays, "rays")))
    pos_ref, rays_ref = dev(ref["pos"]).reshape(-1, 3), dev(ref["rays"]).reshape(-1, 11)
    zero3 = torch.zeros((h, w, 3), device="cuda")
    # mode="point": what ExtractMesh does per vertex
    atlas = texture.BakeTexture(small, r, tile=tile, mode="point", chunk_rows=37)
    raw = r.RunNetwork(pos_ref[:, None, :], rays_ref[:, 3:6].contiguous())
    want = torch.where(owned[..., None], torch.sigmoid(raw[:, 0, :3]).reshape(h, w, 3), zero3)
    assert isinstance(atlas, texture.TextureAtlas) and (atlas.Tile, atlas.NFaces, atlas.Acc) == (tile, nf, None) and atlas.Image.shape == (h, w, 3)
    assert torch.equal(atlas.Image, want) and float(atlas.Image.max()) > 0
    # mode="render": the short rays through BatchifyRays
    rp = scene.lego_render_params(sc["bbox"], n_samples=16, n_importance=16)
    baked = texture.BakeTexture(small, r, tile=tile, mode="render", rparams=rp, offset=offset)
    o = r.BatchifyRays(rays_ref, None, rp.NSamples, chunk=rp.Chunk, n_importance=rp.NImportance, white_bkgr=rp.WhiteBkgr, precision=rp.Precision, return_weights=False).Outputs
    assert torch.equal(baked.Image, torch.where(owned[..., None], o.RGBMap.reshape(h, w, 3), zero3))
    assert torch.equal(baked.Acc, torch.where(owned, o.AccMap.reshape(h, w), zero3[..., 0]))
    slabbed = texture.BakeTexture(small, r, tile=tile, mode="render", rparams=rp, offset=offset, chunk_rows=64)
    assert torch.equal(slabbed.Image, baked.Image) and torch.equal(slabbed.Acc, baked.Acc), "slabs change nothing"
    for kw, match in ((dict(mode="render", rparams=rp), "offset"), (dict(mode="render", offset=offset), "rparams"), (dict(mode="splat"), "mode"),
                      (dict(mode="render", offset=offset, rparams=scene.lego_render_params(sc["bbox"], Ndc=True)), "Ndc")):
        with pytest.raises(L.NrfError, match=match):
            texture.BakeTexture(small, r, tile=tile, **kw)
    with pytest.raises(L.NrfError, match="LeRF"):
        texture.BakeTexture(small, scene.make_lerf_scene(log2_t=14)["renderer"], tile=tile)
    # a TSDF volume: its colour volume at P
    views = tsdf.OrbitViews(4, 24, 24, scene.lego_K(24, 24), 4.0)
    vol = tsdf.FuseViews(r, views, rp, resolution=24)
    from_vol = texture.BakeTexture(small, vol, tile=tile, chunk_rows=50)
    assert torch.equal(from_vol.Image, torch.where(owned[..., None], vol.SampleColor(pos_ref).reshape(h, w, 3), zero3))
    print("acc max", float(baked.Acc.max()), "volume colour max", float(from_vol.Image.max()))
    # EvaluateMesh through the atlas: the mesh's own colours are not needed
    bare = mesh.Mesh(small.Vertices, small.Faces, small.Normals)
    got = raster.EvaluateMesh(bare, r, views, rp, texture=baked)
    assert set(got) == {k for n in ("psnr", "ssim", "depth_error", "iou") for k in (n, "mean_" + n)}
    white = torch.ones((3,), device="cuda")
    for i, v in enumerate(views):
        o = RR.RenderView(r, v.Pose, v.W, v.H, v.K, rp).Outputs
        mr = texture.RenderMeshViewTextured(bare, baked, v, rp)
        plain = raster.RenderMesh(bare, v.Pose, v.W, v.H, v.K, attrs=())
        assert torch.equal(mr.FaceMap, plain.FaceMap) and torch.equal(mr.DepthMap, plain.DepthMap)
        rgb = mr.RGBMap + (1.0 - mr.AccMap)[..., None] * white
        rgb_r, acc_r, depth_r = o.RGBMap.reshape(24, 24, 3), o.AccMap.reshape(24, 24), o.DepthMap.reshape(24, 24)
        a, b = mr.AccMap > 0, acc_r >= 0.5
        both = a & b
        err = (mr.DepthMap - depth_r / acc_r).abs().to(torch.float64)[both]
        assert torch.equal(got["psnr"][i], metrics.PSNR(rgb, rgb_r)) and torch.equal(got["ssim"][i], metrics.SSIM(rgb, rgb_r))
        assert float(got["iou"][i]) == float(both.sum()) / float((a | b).sum())
        assert abs(float(got["depth_error"][i]) - float(err.sum() / both.sum())) <= 1e-12
    for n in ("psnr", "ssim", "depth_error", "iou"):
        assert torch.equal(got["mean_" + n], got[n].mean())
    print({k: v.tolist() for k, v in got.items()})
    with pytest.raises(L.NrfError, match="Colors"):
        raster.EvaluateMesh(bare, r, views, rp)


# ------------------------------------------------------------------------------------ 6. the point of the feature
WAVE = np.array([[7.0, -3.0, 2.0], [-2.0, 6.0, 5.0], [4.0, 3.0, -7.0]])          # column c is the wave vector k of channel c


def colour_field(P):
    """c(P) = 0.5 + 0.5 sin(k . P) per channel: about one period across a face of the 32-face sphere (edge ~ 0.54), so it varies inside every face"""
    return 0.5 + 0.5 * np.sin(np.asarray(P, np.float64) @ WAVE)


def field_errors(verts, faces, c2w, face_map, bary_map, rgb_textured, rgb_vertex):
    """Mean |rgb - c(P)| over the hit pixels for both renders, P the pixel's surface point: FaceMap and the perspective-corrected barycentrics"""
    valid, beta = X.surface_bary(verts, faces, face_map, bary_map, c2w)
    assert np.array_equal(valid, face_map >= 0) and valid.sum() > 300
    P = (beta.astype(np.float64)[..., None] * verts.astype(np.float64)[faces[np.where(valid, face_map, 0)]]).sum(-2)
    truth = colour_field(P)
    return float(np.abs(rgb_textured - truth)[valid].mean()), float(np.abs(rgb_vertex - truth)[valid].mean())


def reference_errors(tile=16):
    """The whole of test 6 on the CPU, through the restatements alone -> (textured, vertex-colour) error"""
    from nerfpp_amd import scene
    verts, faces, normals = sphere(1)
    c2w = scene.pose_spherical(67.0, -35.0, 4.0)
    tx = X.texels(verts, faces, normals, tile, 0.0)
    tex = np.where((tx["face"] >= 0)[..., None], colour_field(tx["pos"]), 0.0).astype(F32)
    ras = R.rasterize(verts, faces, colour_field(verts).astype(F32), SHADE_H, SHADE_W, K_SPHERE, c2w)
    textured = X.shade(verts, faces, ras["face"], ras["bary"], c2w, tex, tile, X.BILINEAR)
    return field_errors(verts, faces, c2w, ras["face"], ras["bary"], textured, ras["attr"])


def test_a_baked_texture_is_closer_to_the_field_than_vertex_colours(api):
    """The 32-face sphere, c(P) = 0.5 + 0.5 sin(k . P) baked at tile 16 through the callable source, and the same c at the vertices as mesh.Colors: the mean absolute
    error of RenderMeshTextured against c at each pixel's surface point must be below that of the vertex-colour RenderMesh.  No bar is invented: the inequality
    itself is the test.  On the CPU, through the restatements alone (reference_errors), the two errors are 0.00266 (textured) and 0.27024 (vertex colours)."""
    L, texture, mesh, scene = api
    from nerfpp_amd import raster
    verts, faces, normals = sphere(1)
    assert len(faces) == 32
    wave = dev(WAVE)
    source = lambda pos, dirs: 0.5 + 0.5 * torch.sin(pos @ wave)
    m = mesh.Mesh(dev(verts), dev(faces, np.int32), dev(normals), dev(colour_field(verts)))
    atlas = texture.BakeTexture(m, source, tile=16)
    assert atlas.Image.shape == (64, 64, 3) and atlas.Acc is None
    c2w = scene.pose_spherical(67.0, -35.0, 4.0)
    textured = texture.RenderMeshTextured(m, atlas, c2w, SHADE_W, SHADE_H, K_SPHERE)
    plain = raster.RenderMesh(m, c2w, SHADE_W, SHADE_H, K_SPHERE, attrs=("Colors",))
    assert torch.equal(textured.FaceMap, plain.FaceMap) and torch.equal(textured.BaryMap, plain.BaryMap)
    e_tex, e_vert = field_errors(verts, faces, c2w, plain.FaceMap.cpu().numpy(), plain.BaryMap.cpu().numpy(), textured.RGBMap.cpu().numpy(), plain.RGBMap.cpu().numpy())
    print(f"textured {e_tex:.5f}  vertex colours {e_vert:.5f}")
    assert e_tex < e_vert
