"""Texture atlases without a GPU: the header, the binding and the Python constants agree; nrf_atlas_dims and the refusals of the device entries (they come before
any device call); the layout's ownership and footprint properties on the numpy restatement (tests/texture_ref.py); the PNG writer and SaveOBJ."""
import ctypes as C
import os
import re
import struct
import zlib

import numpy as np
import pytest
import torch

import raster_ref as R
import texture_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INVALID_ARG = 1
TILES = list(range(4, 13))


def test_header_binding_and_constants_agree():
    from nerfpp_amd import _lib, texture
    hdr = open(os.path.join(ROOT, "include", "nerfpp_hip.h")).read()
    for name, value, mine, ref in (("ATLAS_MIN_TILE", 4, texture.MIN_TILE, X.MIN_TILE), ("ATLAS_MAX_TILE", 64, texture.MAX_TILE, X.MAX_TILE),
                                   ("ATLAS_MAX_SIZE", 16384, texture.MAX_SIZE, X.MAX_SIZE), ("TEXTURE_MAX_CHANNELS", 8, texture.MAX_CHANNELS, X.MAX_CHANNELS),
                                   ("TEXTURE_NEAREST", 0, texture.NEAREST, X.NEAREST), ("TEXTURE_BILINEAR", 1, texture.BILINEAR, X.BILINEAR)):
        m = re.search(rf"#define\s+NRF_{name}\s+(\d+)", hdr)
        assert m and int(m[1]) == value == mine == ref, name
    want = dict(nrf_atlas_dims=("i", "lipp"), nrf_atlas_texels=("i", "plplpifiippppp"), nrf_texture_sample=("i", "pliipplipp"),
                nrf_texture_shade=("i", "plplppiipppiiipp"))
    for fn, sig in want.items():
        assert re.search(rf"NRF_API int {fn}\(", hdr) and _lib.SIGNATURES[fn] == sig, fn
    at = _lib.SYMBOLS.index("nrf_ssim_loss")
    assert _lib.SYMBOLS[at + 1:at + 5] == list(want), "after the image metrics, in the header's order"
    assert hdr.index("nrf_ssim_loss(") < hdr.index("Texture atlases") < hdr.index("nrf_atlas_dims(") < hdr.index("Density gradient")
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, fn) for fn in want)
    import nerfpp_amd
    assert "texture" in nerfpp_amd.__all__ and nerfpp_amd.texture is texture


def test_atlas_dims_and_refusals_need_no_gpu():
    from nerfpp_amd import _lib, texture
    lib = _lib.lib()

    def dims(f, t):
        w, h = C.c_int(-7), C.c_int(-7)
        return lib.nrf_atlas_dims(f, t, C.byref(w), C.byref(h)), w.value, h.value

    for t in (4, 5, 8, 17, 64):
        for f in (0, 1, 2, 3, 7, 8, 9, 128, 129, 511, 512, 513, 11_000, 299_999):
            w, h, cols, rows = X.layout(f, t)
            if max(w, h) > 16384:          # 299 999 faces at tile 64
                assert dims(f, t)[0] == INVALID_ARG and (f, t) == (299_999, 64)
                continue
            assert dims(f, t) == (0, w, h) and texture.AtlasLayout(f, t) == (w, h, cols, rows), (f, t)
            cells = (f + 1) // 2
            assert cols * rows >= cells and (cols == 0 or ((cols - 1) ** 2 < cells <= cols * cols and (rows - 1) * cols < cells))
    assert dims(0, 8) == (0, 0, 0) and dims(1, 8) == (0, 8, 8) and dims(2, 8) == (0, 8, 8) and dims(3, 8) == (0, 16, 8) and dims(7, 4) == (0, 8, 8)
    # the largest atlas: 2 * (16384 / T)^2 faces fit, one more does not, and the message says so
    for t in (4, 16, 17, 64):
        fit = 2 * (16384 // t) ** 2
        assert dims(fit, t) == (0, 16384 // t * t, 16384 // t * t)
        assert dims(fit + 1, t)[0] == INVALID_ARG
        msg = lib.nrf_last_error().decode()
        assert msg.startswith("nrf_atlas_dims") and f"{fit} faces fit" in msg, msg
        with pytest.raises(_lib.NrfError, match=f"{fit} faces fit"):
            texture.AtlasLayout(fit + 1, t)
    for f, t in ((8, 3), (8, 65), (8, 0), (8, -1), (-1, 8), (2 ** 31 - 1, 8)):
        assert dims(f, t) == (INVALID_ARG, -7, -7) and lib.nrf_last_error().startswith(b"nrf_atlas_dims"), (f, t)
        with pytest.raises(_lib.NrfError):
            texture.AtlasLayout(f, t)
    assert lib.nrf_atlas_dims(8, 8, None, None) == INVALID_ARG
    # the device entries refuse before anything touches the device
    fake = C.c_void_p(256)          # never dereferenced: every call below is refused
    K = np.array([[8, 0, 3], [0, 8, 2], [0, 0, 1]], F32)
    pose = R.LATTICE_POSE.copy()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    nan, inf = float("nan"), float("inf")

    def texels(verts=fake, nv=6, faces=fake, nf=8, tile=8, offset=0.0, row0=0, rows=16, face=fake):
        return lib.nrf_atlas_texels(verts, nv, faces, nf, None, tile, offset, row0, rows, face, None, None, None, None)
    for kw in (dict(verts=None), dict(faces=None), dict(face=None), dict(tile=3), dict(tile=65), dict(nf=-1), dict(nf=2 ** 31 - 1), dict(nv=-1), dict(nv=2 ** 31),
               dict(offset=-0.5), dict(offset=nan), dict(offset=inf), dict(row0=-1), dict(rows=-1), dict(rows=17), dict(row0=16, rows=1), dict(nf=2 * 4096 ** 2 + 1, tile=4)):
        assert texels(**kw) == INVALID_ARG and lib.nrf_last_error().startswith(b"nrf_atlas_texels"), (kw, lib.nrf_last_error())
    assert texels(rows=0, face=None) == 0 and texels(nf=0, rows=0) == 0, "an empty window launches nothing"

    def sample(tex=fake, nf=8, tile=8, c=3, face=fake, bary=fake, n=4, flt=1, out=fake):
        return lib.nrf_texture_sample(tex, nf, tile, c, face, bary, n, flt, out, None)
    for kw in (dict(tex=None), dict(face=None), dict(bary=None), dict(out=None), dict(tile=3), dict(tile=65), dict(nf=-1), dict(c=0), dict(c=9), dict(flt=2), dict(flt=-1),
               dict(n=-1)):
        assert sample(**kw) == INVALID_ARG and lib.nrf_last_error().startswith(b"nrf_texture_sample"), (kw, lib.nrf_last_error())
    assert sample(n=0, face=None, bary=None, out=None) == 0

    def shade(verts=fake, nv=6, faces=fake, nf=8, fmap=fake, bmap=fake, h=4, w=4, k=p(K), m=p(pose), tex=fake, tile=8, c=3, flt=1, out=fake):
        return lib.nrf_texture_shade(verts, nv, faces, nf, fmap, bmap, h, w, k, m, tex, tile, c, flt, out, None)
    for kw in (dict(verts=None), dict(faces=None), dict(fmap=None), dict(bmap=None), dict(k=None), dict(m=None), dict(tex=None), dict(out=None), dict(h=0), dict(w=0),
               dict(h=16385), dict(w=16385), dict(tile=3), dict(c=0), dict(c=9), dict(flt=2), dict(nf=-1), dict(nv=-1), dict(nv=2 ** 31)):
        assert shade(**kw) == INVALID_ARG and lib.nrf_last_error().startswith(b"nrf_texture_shade"), (kw, lib.nrf_last_error())


@pytest.mark.parametrize("tile", TILES)
def test_every_texel_has_at_most_one_owner_and_the_counts_match(tile):
    """The baking side (owners: texel -> face and indices) and the sampling side (texel_of: face and indices -> texel) are two statements of one layout: walking every
    face's own index set through texel_of reaches distinct texels, each of which names that face and those indices back, and nothing else is owned."""
    for nf in (0, 1, 2, 7, 128):
        w, h, cols, rows = X.layout(nf, tile)
        face, i, j = X.owners(nf, tile)
        cells = (nf + 1) // 2
        assert face.shape == (h, w) and cols * rows >= cells and (w, h) == (cols * tile, rows * tile)
        lower, upper = (nf + 1) // 2, nf // 2
        assert (face >= 0).sum() == lower * tile * (tile - 1) // 2 + upper * tile * (tile + 1) // 2
        seen = np.zeros((h, w), np.int64)
        for f in range(nf):
            fi, fj = np.mgrid[0:tile, 0:tile]
            own = fi + fj <= (tile - 2 if f % 2 == 0 else tile - 1)
            tx, ty = X.texel_of(nf, tile, np.full(own.sum(), f), fi[own], fj[own])
            assert (tx >= 0).all() and (tx < w).all() and (ty >= 0).all() and (ty < h).all()
            assert (face[ty, tx] == f).all() and (i[ty, tx] == fi[own]).all() and (j[ty, tx] == fj[own]).all()
            assert np.array_equal(np.bincount(face[face >= 0], minlength=nf)[f], own.sum())
            np.add.at(seen, (ty, tx), 1)
        assert np.array_equal(seen, (face >= 0).astype(np.int64)), "every owned texel is reached exactly once, no other texel at all"
        if nf % 2 == 1:
            last = X.texel_of(nf, tile, np.array([nf]), np.array([0]), np.array([0]))          # where face F would start: the upper half of the last cell
            assert face[last[1][0], last[0][0]] == -1


def lattice(m):
    """All barycentrics (b0, b1, b2) = (m - a - b, a, b) / m of a face, edges and corners included, as fp32"""
    a, b = np.mgrid[0:m + 1, 0:m + 1]
    keep = a + b <= m
    a, b = a[keep].astype(np.float64), b[keep].astype(np.float64)
    return np.stack([(m - a - b) / m, a / m, b / m], -1).astype(F32)


@pytest.mark.parametrize("tile", TILES)
def test_a_bilinear_footprint_reads_only_the_faces_own_texels(tile):
    """Both halves of a cell and a cell off the first row (faces 0, 1 and 6 of 7; 6 is the last face of an odd count).  Every other texel holds NaN, so a fetch outside
    the face would also show in the value; the texels of the face hold a function linear in its indices, which bilinear filtering must give back."""
    nf, n = 7, tile - 3
    face, i, j = X.owners(nf, tile)
    for f in (0, 1, 6):
        for m in (n, 2 * n, 24, 7 * n + 1):
            bary = lattice(m)
            tex = np.where((face == f)[..., None], np.stack([0.25 + i * 0.5 + j * 2.0, 3.0 - i + 0.125 * j], -1), np.nan).astype(F32)
            for flt in (X.BILINEAR, X.NEAREST):
                trace = []
                out = X.sample(tex, nf, tile, np.full(len(bary), f), bary, flt, trace)
                assert len(trace) == (4 if flt == X.BILINEAR else 1)
                for tx, ty, read in trace:
                    assert read.any() and (face[ty[read], tx[read]] == f).all(), (f, m, flt)
                assert np.isfinite(out).all(), (f, m, flt)
                x, y = bary[:, 1].astype(np.float64) * n, bary[:, 2].astype(np.float64) * n
                if flt == X.BILINEAR:
                    want = np.stack([0.25 + x * 0.5 + y * 2.0, 3.0 - x + 0.125 * y], -1)
                    assert np.abs(out - want).max() <= 4e-6 * (3.0 + 2.5 * n), (f, m)
                else:
                    want = np.stack([0.25 + np.rint(x) * 0.5 + np.rint(y) * 2.0, 3.0 - np.rint(x) + 0.125 * np.rint(y)], -1)
                    exact = (np.abs(x - np.rint(x)) < 0.49) & (np.abs(y - np.rint(y)) < 0.49)          # away from the rounding ties of fp32 b * n
                    assert exact.sum() > 0 and np.array_equal(out[exact], want[exact].astype(F32)), (f, m)
    # the statement of the header: the corners a point of the face reads have i + j <= n + 1 = tile - 2, inside the lower face's own i + j <= tile - 2
    assert n + 1 == tile - 2


def decode_png(data):
    """A PNG decoder for what EncodePNG writes (8-bit RGB, no interlace), every chunk's CRC checked, all five row filters understood -> [H, W, 3] uint8"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        (n,), kind = struct.unpack(">I", data[at:at + 4]), data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        chunks.append((kind, body))
        at += 12 + n
    assert at == len(data) and chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, flt, lace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(b"".join(body for kind, body in chunks if kind == b"IDAT"))
    assert len(raw) == h * (1 + 3 * w)
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + 3 * w)
    out = np.zeros((h, 3 * w), np.int64)
    for r in range(h):
        kind, line = int(rows[r, 0]), rows[r, 1:].astype(np.int64)
        up = out[r - 1] if r else np.zeros(3 * w, np.int64)
        assert 0 <= kind <= 4
        if kind in (0, 2):
            out[r] = (line + (up if kind == 2 else 0)) & 255
            continue
        for k in range(3 * w):
            a = out[r, k - 3] if k >= 3 else 0
            c = up[k - 3] if k >= 3 else 0
            if kind == 1:
                pred = a
            elif kind == 3:
                pred = (a + up[k]) // 2
            else:
                pa, pb, pc = abs(up[k] - c), abs(a - c), abs(a + up[k] - 2 * c)
                pred = a if pa <= pb and pa <= pc else up[k] if pb <= pc else c
            out[r, k] = (line[k] + pred) & 255
    return out.astype(np.uint8).reshape(h, w, 3)


def test_png_writer_round_trips():
    from nerfpp_amd import texture
    rng = np.random.default_rng(3)
    for h, w in ((1, 1), (1, 7), (5, 1), (24, 40), (64, 64)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if (h, w) == (64, 64):
            img[:, :32] = 200          # something that compresses
        data = texture.EncodePNG(img)
        assert isinstance(data, bytes) and np.array_equal(decode_png(data), img), (h, w)
    q = texture.QuantizeTexture(torch.tensor([[[0.0, 1.0, 0.5], [-0.25, 1.5, 0.25], [float("nan"), 0.498, 0.002]]]))
    assert q.tolist() == [[[0, 255, 128], [0, 255, 64], [0, 127, 1]]]          # clamp(round(255 c)), half to even, NaN as 0
    assert texture.QuantizeTexture(torch.tensor([[[0.5]]])).tolist() == [[[128, 128, 128]]]


@pytest.mark.parametrize("n_faces,tile", [(8, 4), (7, 5), (31, 8), (1, 17)])
def test_save_obj_puts_every_vt_on_the_texel_centre_the_layout_names(tmp_path, n_faces, tile):
    from nerfpp_amd import _lib, mesh, texture
    verts, faces = R.octa_sphere((0.0, 0.0, 0.0), 1.0, levels=1)
    faces = faces[:n_faces]
    w, h, _, _ = X.layout(n_faces, tile)
    image = torch.from_numpy(np.random.default_rng(5).uniform(-0.1, 1.1, (h, w, 3)).astype(F32))
    m = mesh.Mesh(torch.from_numpy(verts), torch.from_numpy(faces), torch.from_numpy(verts.copy()))
    atlas = texture.TextureAtlas(image, tile, n_faces)
    path = str(tmp_path / "ball.obj")
    texture.SaveOBJ(path, m, atlas)
    rows = [line.split() for line in open(path).read().splitlines()]
    v = np.array([r[1:] for r in rows if r[0] == "v"], np.float64)
    vn = np.array([r[1:] for r in rows if r[0] == "vn"], np.float64)
    vt = np.array([r[1:] for r in rows if r[0] == "vt"], np.float64)
    f = np.array([[[int(x) for x in c.split("/")] for c in r[1:]] for r in rows if r[0] == "f"])
    assert np.array_equal(v.astype(F32), verts) and np.array_equal(vn.astype(F32), verts) and vt.shape == (3 * n_faces, 2) and f.shape == (n_faces, 3, 3)
    assert np.array_equal(f[..., 0] - 1, faces) and np.array_equal(f[..., 2], f[..., 0]) and np.array_equal(f[..., 1].reshape(-1), np.arange(3 * n_faces) + 1)
    assert ["mtllib", "ball.obj.mtl"] in rows and "map_Kd ball.obj.png" in open(path + ".mtl").read()
    # every vt is a texel centre; that texel belongs to the face, at the indices of the corner
    tx, ty = vt[:, 0] * w - 0.5, (1.0 - vt[:, 1]) * h - 0.5
    assert np.abs(tx - np.rint(tx)).max() <= 1e-9 and np.abs(ty - np.rint(ty)).max() <= 1e-9
    tx, ty = np.rint(tx).astype(np.int64).reshape(-1, 3), np.rint(ty).astype(np.int64).reshape(-1, 3)
    face, i, j = X.owners(n_faces, tile)
    n = tile - 3
    assert np.array_equal(face[ty, tx], np.repeat(np.arange(n_faces)[:, None], 3, 1))
    assert np.array_equal(i[ty, tx], np.tile([0, n, 0], (n_faces, 1))) and np.array_equal(j[ty, tx], np.tile([0, 0, n], (n_faces, 1)))
    # the corners are where the baked barycentrics say: texel (i, j) = (n, 0) has b1 = 1, (0, n) has b2 = 1
    ref = X.texels(verts, faces, None, tile, 0.0)
    assert np.array_equal(ref["bary"][ty, tx], np.tile(np.eye(3, dtype=F32), (n_faces, 1, 1)))
    assert np.abs(ref["pos"][ty, tx] - verts[faces]).max() <= 2.5e-7, "v0 + (v1 - v0) is v1 up to two roundings of coordinates <= 1"
    # the PNG holds the quantised atlas
    png = decode_png(open(path + ".png", "rb").read())
    assert np.array_equal(png, np.clip(np.rint(image.numpy().astype(np.float64) * 255.0), 0, 255).astype(np.uint8))
    with pytest.raises(_lib.NrfError, match="one face order"):
        texture.SaveOBJ(path, mesh.Mesh(m.Vertices, m.Faces[:-1] if n_faces > 1 else torch.cat([m.Faces, m.Faces]), m.Normals), atlas)
    with pytest.raises(_lib.NrfError, match="TextureAtlas"):
        texture.TextureAtlas(image[:-1], tile, n_faces)
