"""Time the LeRF relevancy query on one MI355X: a 256^3 RelevancyGrid (sigma_le included) on the main.cpp-size LeRF scene (scene.make_lerf_scene()), fused
NRF_PREC_F16_SPLIT against the NRF_PREC_F32 composed path (nrf_mlp_forward(F32) in chunks, normalise, relevancy) on the same lattice.

Warm-up first, then hipEvent timing of each call and the median of the repeats (one JSON line on stdout; --out also writes it to a file).
    python tools/lerf_query_bench.py [--res 256] [--repeats 10] [--f32-repeats 3] [--out FILE]
"""
import argparse
import json
import os
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--f32-repeats", type=int, default=3)
    ap.add_argument("--n-neg", type=int, default=4)
    ap.add_argument("--skip-f32", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nerfpp_amd import _lib as L, query, scene
    torch.cuda.set_device(0)
    sc = scene.make_lerf_scene()
    r = sc["renderer"]
    rng = np.random.default_rng(5)
    pr = rng.standard_normal((1 + a.n_neg, 768))
    pr = (pr / np.linalg.norm(pr, axis=1, keepdims=True)).astype(np.float32)
    r.SetLeRFPrompts(pr[:1], pr[1:])
    res = a.res
    out = dict(lattice=res, points=res ** 3, n_neg=a.n_neg)
    fused = lambda: query.RelevancyGrid(r, resolution=res, precision=L.NRF_PREC_F16_SPLIT)
    out["fused_split_ms"], out["fused_split_all_ms"] = timed(fused, 2, a.repeats)
    out["fused_mfma_ms"], _ = timed(lambda: query.RelevancyGrid(r, resolution=res, precision=L.NRF_PREC_F16_MFMA), 1, a.repeats)
    out["fused_split_ns_per_point"] = out["fused_split_ms"] * 1e6 / res ** 3
    if not a.skip_f32:
        out["composed_f32_ms"], out["composed_f32_all_ms"] = timed(lambda: query.RelevancyGrid(r, resolution=res, precision=L.NRF_PREC_F32), 1, a.f32_repeats)
        out["speedup_vs_f32"] = out["composed_f32_ms"] / out["fused_split_ms"]
        rs, ss = fused()
        rf, sf = query.RelevancyGrid(r, resolution=res, precision=L.NRF_PREC_F32)
        out["max_abs_rel_split_vs_f32"] = float((rs - rf).abs().max())
        out["sigma_bit_equal"] = bool(torch.equal(ss.view(torch.int32), sf.view(torch.int32)))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
