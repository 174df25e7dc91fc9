"""numpy restatement of the depth fusion's contract (include/nerfpp_hip.h, nrf_tsdf_integrate / nrf_tsdf_observed / nrf_tsdf_sample_color): one numpy fp32 operation
per source operation of the kernels, vectorised over the lattice, so the GPU output is compared with this bit for bit.  Also the analytic sphere scene the host
tests pin the definition on, and the host twin of TSDFVolume.Extract (mesh_ref.isosurface + the observed filter)."""
import numpy as np

import mesh_ref as M

F32 = np.float32
CLASSES = ("updated", "carved", "behind", "outside", "bad_depth", "nan_acc", "below_trunc", "colour_skipped", "weight_clamped")


def new_volume(nx, ny, nz, colors=True):
    """(tsdf = 1, weight = 0, color = 0 or None)"""
    return np.ones((nz, ny, nx), F32), np.zeros((nz, ny, nx), F32), (np.zeros((4, nz, ny, nx), F32) if colors else None)


def _steps(bbox, nx, ny, nz):
    b = np.asarray(bbox, F32).reshape(6)
    return b, [(b[3 + a] - b[a]) / F32(n - 1) for a, n in enumerate((nx, ny, nz))]


def integrate(tsdf, weight, color, bbox, views, trunc, acc_min, max_weight, carve, counts=None):
    """In place.  views: dicts of depth [h, w], K [3, 3], c2w [3, 4] and optionally acc [h, w], rgb [h, w, 3] (absent or None: the NULL of the C entry), taken in order.
    counts: a dict that receives the number of voxel-view pairs of each of CLASSES."""
    nz, ny, nx = tsdf.shape
    P = M.lattice_points(bbox, nx, ny, nz)
    trunc, acc_min, max_weight, one, half, zero = F32(trunc), F32(acc_min), F32(max_weight), F32(1), F32(0.5), F32(0)
    if counts is not None:
        counts.update({k: counts.get(k, 0) for k in CLASSES})
    with np.errstate(all="ignore"):
        for view in views:
            depth = np.asarray(view["depth"], F32)
            acc = None if view.get("acc") is None else np.asarray(view["acc"], F32)
            rgb = None if view.get("rgb") is None else np.asarray(view["rgb"], F32)
            h, w = depth.shape
            K = np.asarray(view["K"], F32).reshape(3, 3)
            c2w = np.asarray(view["c2w"], F32)[:3, :4]
            fx, cx, fy, cy = K[0, 0], K[0, 2], K[1, 1], K[1, 2]
            R, t = c2w[:, :3], c2w[:, 3]
            # 1. camera coordinates
            qx, qy, qz = P[..., 0] - t[0], P[..., 1] - t[1], P[..., 2] - t[2]
            xc = (R[0, 0] * qx + R[1, 0] * qy) + R[2, 0] * qz
            yc = (R[0, 1] * qx + R[1, 1] * qy) + R[2, 1] * qz
            zc = (R[0, 2] * qx + R[1, 2] * qy) + R[2, 2] * qz
            zd = -zc
            front = zd > zero
            # 2. pixel
            u = fx * (xc / zd) + cx
            v = cy - fy * (yc / zd)
            fu, fv = np.floor(u + half), np.floor(v + half)
            inimg = front & (fu >= zero) & (fu < F32(w)) & (fv >= zero) & (fv < F32(h))
            px, py = np.where(inimg, fu, zero).astype(np.int64), np.where(inimg, fv, zero).astype(np.int64)
            # 3. depth
            d = depth[py, px]
            if acc is not None:
                a = acc[py, px]
                solid = inimg & (a >= acc_min)
                carved = inimg & (a < acc_min) & bool(carve)
                d = np.where(solid, d / a, d)
                nan_acc = inimg & np.isnan(a)
            else:
                solid, carved, nan_acc = inimg, np.zeros_like(inimg), np.zeros_like(inimg)
            good = solid & np.isfinite(d) & (d > zero)
            # 4. signed distance
            sdf = d - zd
            below = good & (sdf < -trunc)
            surface = good & ~below
            s = np.where(carved, one, np.minimum(one, sdf / trunc))
            # 5. update
            upd = surface | carved
            Wn = weight + one
            newD = (tsdf * weight + s) / Wn
            clamped = upd & (Wn > max_weight)
            tsdf[...] = np.where(upd, newD, tsdf)
            weight[...] = np.where(upd, np.minimum(Wn, max_weight), weight)
            # 6. colour
            far = surface & ~(np.abs(sdf) <= trunc)
            if color is not None and rgb is not None:
                cm = surface & ~far
                cw = color[3]
                cn = cw + one
                for ch in range(3):
                    color[ch] = np.where(cm, (color[ch] * cw + rgb[py, px, ch]) / cn, color[ch])
                color[3] = np.where(cm, np.minimum(cn, max_weight), cw)
            if counts is not None:
                for k, m in zip(CLASSES, (surface, carved, ~front, front & ~inimg, solid & ~good, nan_acc, below, far, clamped)):
                    counts[k] += int(m.sum())


def observed(weight, bbox, pts):
    """[p] bool"""
    nz, ny, nx = weight.shape
    b, step = _steps(bbox, nx, ny, nz)
    pts = np.asarray(pts, F32).reshape(-1, 3)
    n = (nx, ny, nz)
    with np.errstate(all="ignore"):
        r = [np.fmin(np.fmax(np.floor((pts[:, a] - b[a]) / step[a] + F32(0.5)), F32(-1)), F32(n[a])).astype(np.int64) for a in range(3)]
    ok = np.isfinite(pts).all(-1)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ok = ok & (weight[np.clip(r[2] + dz, 0, nz - 1), np.clip(r[1] + dy, 0, ny - 1), np.clip(r[0] + dx, 0, nx - 1)] > 0)
    return ok


def sample_color(color, bbox, pts):
    """[p, 3] f32"""
    _, nz, ny, nx = color.shape
    b, step = _steps(bbox, nx, ny, nz)
    pts = np.asarray(pts, F32).reshape(-1, 3)
    n = (nx, ny, nz)
    i0, f = [], []
    with np.errstate(all="ignore"):
        for a in range(3):
            g = (pts[:, a] - b[a]) / step[a]
            fl = np.fmin(np.fmax(np.floor(g), F32(0)), F32(n[a] - 2))
            i0.append(fl.astype(np.int64))
            f.append(np.fmin(np.fmax(g - fl, F32(0)), F32(1)))
        den = np.zeros(len(pts), F32)
        num = np.zeros((3, len(pts)), F32)
        for c in range(8):
            bx, by, bz = c & 1, c >> 1 & 1, c >> 2
            wx, wy, wz = (f[0] if bx else F32(1) - f[0]), (f[1] if by else F32(1) - f[1]), (f[2] if bz else F32(1) - f[2])
            lam = (wx * wy) * wz
            j = (i0[2] + bz, i0[1] + by, i0[0] + bx)
            has = color[3][j] > 0
            den = np.where(has, den + lam, den)
            for k in range(3):
                num[k] = np.where(has, num[k] + lam * color[k][j], num[k])
        out = np.where(den == 0, F32(0), num / den)
    return np.ascontiguousarray(out.T.astype(F32))


def submesh(verts, faces, normals, keep_faces):
    """mesh._submesh: the vertices the kept faces use in ascending original order, faces re-indexed -> (verts, faces, normals, old vertex ids)"""
    fk = faces[keep_faces]
    old = np.unique(fk)
    remap = np.full(len(verts), -1, np.int64)
    remap[old] = np.arange(len(old))
    return verts[old], remap[fk].astype(np.int32), normals[old], old


def extract(tsdf, weight, bbox, filtered=True):
    """TSDFVolume.Extract on the host -> (verts, faces, normals)"""
    v, f, n, _ = M.isosurface(-tsdf, bbox, F32(0))
    if not filtered:
        return v, f, n
    ok = observed(weight, bbox, v)
    return submesh(v, f, n, ok[f].all(-1))[:3]


# ---- the analytic scene of the host tests: a sphere seen by a ring of pinhole cameras ----
SPHERE = dict(centre=(0.1, -0.15, 0.2), radius=0.7, bbox=np.array([-1.5, -1.5, -1.5, 1.5, 1.5, 1.5], F32), n=33, h=48, w=56, n_views=6, trunc_steps=4.0,
              acc_min=0.5, max_weight=64.0)


def sphere_depth(h, w, K, c2w, radius, centre):
    """(depth, acc) [h, w] f32 of the closed-form ray-sphere intersection in float64 along the rays of GetRays (dx = (x - cx) / fx, dy = -(y - cy) / fy, dz = -1):
    acc = 1 on a hit, depth = acc * t as a render's sum of w z is"""
    K = np.asarray(K, np.float64)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    d = np.stack([(x - K[0, 2]) / K[0, 0], -(y - K[1, 2]) / K[1, 1], -np.ones_like(x)], -1)
    R = np.asarray(c2w, np.float64)[:, :3]
    o = np.asarray(c2w, np.float64)[:, 3] - np.asarray(centre, np.float64)
    dw = d @ R.T
    a, b, c = (dw * dw).sum(-1), 2 * (dw @ o), o @ o - radius * radius
    disc = b * b - 4 * a * c
    hit = disc > 0
    t = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0))) / (2 * a), 0.0)
    acc = hit.astype(F32)
    return (t * acc).astype(F32), acc


def sphere_views(pose_spherical, lego_K):
    """The 6 views of the host test (scene.pose_spherical / scene.lego_K are handed in: this module imports nothing of the package); rgb is a smooth function of the
    pixel, so the colour volume has something to hold."""
    s = SPHERE
    K = lego_K(s["h"], s["w"])
    views = []
    for i in range(s["n_views"]):
        c2w = pose_spherical(60.0 * i + 7.0, -35.0 if i % 2 else 25.0, 4.0)
        depth, acc = sphere_depth(s["h"], s["w"], K, c2w, s["radius"], s["centre"])
        y, x = np.mgrid[0:s["h"], 0:s["w"]].astype(F32)
        rgb = np.stack([x / F32(s["w"]), y / F32(s["h"]), np.full_like(x, F32(i) / F32(s["n_views"]))], -1).astype(F32)
        views.append(dict(depth=depth, acc=acc, rgb=rgb, K=K, c2w=c2w))
    return views


def sphere_step():
    s = SPHERE
    return float((s["bbox"][3] - s["bbox"][0]) / F32(s["n"] - 1))


def fuse_sphere(views, carve=True, colors=True):
    s = SPHERE
    tsdf, weight, color = new_volume(s["n"], s["n"], s["n"], colors)
    integrate(tsdf, weight, color, s["bbox"], views, F32(s["trunc_steps"]) * F32(sphere_step()), s["acc_min"], s["max_weight"], carve)
    return tsdf, weight, color


def radial_error(verts):
    """| |v - c| - r | in lattice steps"""
    s = SPHERE
    rad = np.linalg.norm(verts.astype(np.float64) - np.asarray(s["centre"], np.float64), axis=1)
    return np.abs(rad - s["radius"]) / sphere_step()
