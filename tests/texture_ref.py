"""numpy restatement of the texture-atlas contract (include/nerfpp_hip.h: the layout, nrf_atlas_texels, nrf_texture_sample, nrf_texture_shade), written from the
header: one numpy fp32 operation per source operation, so the GPU output is compared with this bit for bit.  Imports nothing of the package."""
import math

import numpy as np

F32 = np.float32
MIN_TILE, MAX_TILE, MAX_SIZE, MAX_CHANNELS = 4, 64, 16384, 8
NEAREST, BILINEAR = 0, 1


def layout(n_faces, tile):
    """-> (width, height, cols, rows)"""
    assert MIN_TILE <= tile <= MAX_TILE and n_faces >= 0
    cells = (n_faces + 1) // 2
    cols = math.isqrt(cells)
    if cols * cols < cells:
        cols += 1
    rows = (cells + cols - 1) // cols if cells else 0
    return cols * tile, rows * tile, cols, rows


def owners(n_faces, tile):
    """-> (face [H, W] int64, -1 where the texel has no owner; i, j [H, W]: the texel's indices in its face's own frame)"""
    w, h, cols, _ = layout(n_faces, tile)
    Y, X = np.mgrid[0:h, 0:w].astype(np.int64)
    i, j = X % tile, Y % tile
    cell = (X // tile) + cols * (Y // tile)
    upper = i + j > tile - 2
    i, j = np.where(upper, tile - 1 - i, i), np.where(upper, tile - 1 - j, j)
    f = 2 * cell + upper
    return np.where(f < n_faces, f, -1), i, j


def texel_of(n_faces, tile, f, i, j):
    """(X, Y) of the texel with the indices (i, j) of face f"""
    _, _, cols, _ = layout(n_faces, tile)
    f = np.asarray(f, np.int64)
    cell, odd = f >> 1, (f & 1) == 1
    x0, y0 = (cell % cols) * tile, (cell // cols) * tile
    return np.where(odd, x0 + tile - 1 - i, x0 + i), np.where(odd, y0 + tile - 1 - j, y0 + j)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _length(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def texels(verts, faces, normals, tile, offset):
    """nrf_atlas_texels over the whole atlas -> dict(face [H, W] i32, bary [H, W, 3], pos [H, W, 3], rays [H, W, 11])"""
    verts = np.asarray(verts, F32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    nv, nf = len(verts), len(faces)
    face, i, j = owners(nf, tile)
    h, w = face.shape
    if nf == 0:
        return dict(face=face.astype(np.int32), bary=np.zeros((h, w, 3), F32), pos=np.zeros((h, w, 3), F32), rays=np.zeros((h, w, 11), F32))
    fv = faces[np.maximum(face, 0)]
    bad = ((fv < 0) | (fv >= nv)).any(-1)
    face = np.where(bad, -1, face)
    g = np.where((face < 0)[..., None], 0, fv)
    if nv == 0:
        verts = np.zeros((1, 3), F32)
    offset = F32(offset)
    with np.errstate(all="ignore"):
        p0 = verts[g[..., 0]]
        e1, e2 = verts[g[..., 1]] - p0, verts[g[..., 2]] - p0
        c = _cross(e1, e2)
        ln = _length(c)
        face = np.where(ln > 0, face, -1)
        n = F32(tile - 3)
        b1, b2 = i.astype(F32) / n, j.astype(F32) / n
        b0 = (F32(1) - b1) - b2
        P = p0 + (b1[..., None] * e1 + b2[..., None] * e2)
        N = c / ln[..., None]
        if normals is not None:
            nm = np.asarray(normals, F32).reshape(-1, 3) if nv else np.zeros((1, 3), F32)
            m = (b0[..., None] * nm[g[..., 0]] + b1[..., None] * nm[g[..., 1]]) + b2[..., None] * nm[g[..., 2]]
            l = _length(m)
            N = np.where((l > 0)[..., None], m / l[..., None], N)
        rays = np.concatenate([P + offset * N, -N, np.zeros((h, w, 1), F32), np.full((h, w, 1), F32(2) * offset, F32), -N], -1)
    own = (face >= 0)[..., None]
    z = F32(0)
    out = dict(face=face.astype(np.int32), bary=np.where(own, np.stack([b0, b1, b2], -1), z), pos=np.where(own, P, z), rays=np.where(own, rays, z))
    assert all(out[k].dtype == F32 for k in ("bary", "pos", "rays"))
    return out


def sample(tex, n_faces, tile, face, bary, filter, trace=None):
    """nrf_texture_sample -> [p, C] f32.  trace: a list that receives (X, Y, read) per texel fetch: the coordinates and which points fetched there."""
    tex = np.asarray(tex, F32)
    face = np.asarray(face, np.int64).reshape(-1)
    bary = np.asarray(bary, F32).reshape(-1, 3)
    C = tex.shape[2]
    valid = (face >= 0) & (face < n_faces)
    f = np.where(valid, face, 0)
    n = tile - 3
    nf = F32(n)
    with np.errstate(all="ignore"):
        x, y = bary[:, 1] * nf, bary[:, 2] * nf
        x, y = np.where(x > 0, x, F32(0)), np.where(y > 0, y, F32(0))
        x, y = np.where(x > nf, nf, x), np.where(y > nf, nf, y)

        def fetch(i, j, read):
            X, Y = texel_of(n_faces, tile, f, i, j)
            X, Y = np.where(read, X, 0), np.where(read, Y, 0)
            if trace is not None:
                trace.append((X, Y, read))
            return tex[Y, X] if tex.size else np.zeros((len(f), C), F32)

        if filter == NEAREST:
            i, j = np.rint(x).astype(np.int64), np.rint(y).astype(np.int64)
            j = np.where(i + j > n + 1, n + 1 - i, j)
            out = fetch(i, j, valid)
        else:
            assert filter == BILINEAR
            ix, iy = np.floor(x), np.floor(y)
            fx, fy = x - ix, y - iy
            gx, gy = F32(1) - fx, F32(1) - fy
            i0, j0 = ix.astype(np.int64), iy.astype(np.int64)
            out = np.zeros((len(f), C), F32)
            for di, dj, wgt in ((0, 0, gx * gy), (1, 0, fx * gy), (0, 1, gx * fy), (1, 1, fx * fy)):
                i, j = i0 + di, j0 + dj
                read = valid & (i + j <= n + 1)
                out = np.where(read[:, None], out + wgt[:, None] * fetch(i, j, read), out)
    out = np.where(valid[:, None], out, F32(0)).astype(F32)
    return out


def corner_depths(verts, c2w):
    """zd per vertex by step 1 of nrf_raster_mesh"""
    P = np.asarray(verts, F32).reshape(-1, 3)
    c2w = np.asarray(c2w, F32)[:3, :4]
    R, t = c2w[:, :3], c2w[:, 3]
    with np.errstate(all="ignore"):
        qx, qy, qz = P[:, 0] - t[0], P[:, 1] - t[1], P[:, 2] - t[2]
        zc = (R[0, 2] * qx + R[1, 2] * qy) + R[2, 2] * qz
        return -zc


def surface_bary(verts, faces, face_map, bary_map, c2w):
    """Steps 1-3 of nrf_texture_shade -> (valid [h, w], beta [h, w, 3] f32)"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    nv = len(np.asarray(verts).reshape(-1, 3))
    face_map = np.asarray(face_map, np.int64)
    valid = (face_map >= 0) & (face_map < len(faces))
    fv = faces[np.where(valid, face_map, 0)] if len(faces) else np.zeros(face_map.shape + (3,), np.int64)
    valid &= ((fv >= 0) & (fv < nv)).all(-1)
    fv = np.where(valid[..., None], fv, 0)
    zd = corner_depths(verts, c2w) if nv else np.ones(1, F32)
    with np.errstate(all="ignore"):
        p = np.asarray(bary_map, F32) * (F32(1) / zd[fv])
        S = (p[..., 0] + p[..., 1]) + p[..., 2]
        beta = p / S[..., None]
    return valid, beta.astype(F32)


def shade(verts, faces, face_map, bary_map, c2w, tex, tile, filter):
    """nrf_texture_shade -> [h, w, C] f32"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    valid, beta = surface_bary(verts, faces, face_map, bary_map, c2w)
    h, w = valid.shape
    f = np.where(valid, np.asarray(face_map, np.int64), -1)
    return sample(tex, len(faces), tile, f.reshape(-1), beta.reshape(-1, 3), filter).reshape(h, w, -1)
