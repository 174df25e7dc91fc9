"""Time connected-component labelling on one MI355X, on what the library itself produces from the bench hash scene (make_hash_scene(), level = the 0.7 quantile of
the density, the noise-like worst case of DESIGN §8b): nrf_mesh_components on the Isosurface output and nrf_lattice_components (connectivity 14) on the thresholded
density lattice, at each --res.  Beside each time the bytes the algorithm must touch: 12 B per face plus two 4 B passes per vertex (parent, label) for the mesh,
1 B + two 4 B passes per lattice point for the lattice.

Warm-up first, then hipEvent timing of each call (its one stream synchronisation included) and the median of the repeats.  --host-res R also times the way a user had
to do it at R^3: faces to the host plus scipy.sparse.csgraph.connected_components where scipy imports, otherwise torch min-label propagation to convergence (once,
wall clock).  One JSON line on stdout; --out also writes it to a file.
    python tools/components_bench.py [--res 256 512] [--repeats 5] [--warmup 2] [--host-res 256] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), ms


def lattice_call(mask):
    """nrf_lattice_components (connectivity 14) on mask [nz, ny, nx] uint8 with buffers allocated once: (call, result) -- result() = (labels, K of the last call)."""
    import ctypes as C
    from nerfpp_amd import _lib as L
    lib = L.lib()
    nz, ny, nx = mask.shape
    labels = torch.empty(mask.shape, device=mask.device, dtype=torch.int32)
    ws = torch.empty((int(lib.nrf_lattice_components_workspace_bytes(nx, ny, nz)),), device=mask.device, dtype=torch.uint8)
    k = C.c_int64()
    stream = torch.cuda.current_stream().cuda_stream
    return (lambda: L.check(lib.nrf_lattice_components(mask.data_ptr(), nx, ny, nz, 14, labels.data_ptr(), C.byref(k), ws.data_ptr(), ws.numel(), stream)),
            lambda: (labels, k.value))


def mesh_call(faces, n_verts):
    """nrf_mesh_components likewise."""
    import ctypes as C
    from nerfpp_amd import _lib as L
    lib = L.lib()
    labels = torch.empty((n_verts,), device=faces.device, dtype=torch.int32)
    ws = torch.empty((int(lib.nrf_mesh_components_workspace_bytes(n_verts, faces.shape[0])),), device=faces.device, dtype=torch.uint8)
    k = C.c_int64()
    stream = torch.cuda.current_stream().cuda_stream
    return (lambda: L.check(lib.nrf_mesh_components(faces.data_ptr(), n_verts, faces.shape[0], labels.data_ptr(), C.byref(k), ws.data_ptr(), ws.numel(), stream)),
            lambda: (labels, k.value))


def host_way(faces, n_verts):
    """(seconds, K, how): the components of the face graph without the library."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        f = faces.to(torch.int64)
        a, b = torch.cat([f[:, 0], f[:, 1]]), torch.cat([f[:, 1], f[:, 2]])
        label = torch.arange(n_verts, device=f.device)
        rounds = 0
        while True:
            lo = torch.minimum(label[a], label[b])
            new = label.scatter_reduce(0, a, lo, "amin").scatter_reduce(0, b, lo, "amin")
            rounds += 1
            if torch.equal(new, label):
                break
            label = new
        used = torch.zeros(n_verts, dtype=torch.bool, device=f.device)
        used[f.reshape(-1)] = True
        k = int(torch.unique(label[used]).numel())
        torch.cuda.synchronize()
        return time.perf_counter() - t0, k, f"torch min-label propagation, {rounds} rounds"
    f = faces.cpu().numpy()
    t_copy = time.perf_counter() - t0
    a, b = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
    g = sp.coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n_verts, n_verts))
    _, lab = connected_components(g, directed=False)
    k = len(np.unique(lab[np.unique(f)]))
    return time.perf_counter() - t0, k, f"faces to host ({t_copy:.2f} s) + scipy.sparse.csgraph.connected_components"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-res", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nerfpp_amd import mesh as M, scene as S
    torch.cuda.set_device(0)
    sc = S.make_hash_scene()
    out = dict(repeats=a.repeats, warmup=a.warmup, connectivity=14)
    for res in a.res:
        sigma = M.DensityGrid(sc["renderer"], None, res)
        iso = float(torch.quantile(sigma.reshape(-1)[::97].float(), 0.7))
        mask = (sigma > iso).to(torch.uint8)
        row = dict(iso=iso, set_points=int(mask.sum()))
        call, result = lattice_call(mask)
        row["lattice_ms"], row["lattice_all_ms"] = timed(call, a.warmup, a.repeats)
        row["lattice_components"] = result()[1]
        row["lattice_bytes"] = 9 * res ** 3
        del mask, call, result
        verts, faces, _ = M.Isosurface(sigma, sc["bbox"], iso)
        del sigma
        v, f = int(verts.shape[0]), int(faces.shape[0])
        del verts
        row.update(n_verts=v, n_faces=f, mesh_bytes=12 * f + 8 * v)
        call, result = mesh_call(faces, v)
        row["mesh_ms"], row["mesh_all_ms"] = timed(call, a.warmup, a.repeats)
        row["mesh_components"] = result()[1]
        del call, result
        for kind in ("lattice", "mesh"):
            row[f"{kind}_gb_per_s"] = row[f"{kind}_bytes"] / row[f"{kind}_ms"] * 1e-6
        if res == a.host_res:
            row["host_way_s"], k, row["host_way"] = host_way(faces, v)
            assert k == row["mesh_components"], (k, row["mesh_components"])
        out[str(res)] = row
        del faces
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
