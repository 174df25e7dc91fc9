"""Child process of tests/test_hash_backward_gpu.py::test_thread_per_segment_walk_at_4_and_8_features.  nrf_hash_backward_rays reads NRF_HASH_BWD_FEATURE_LANES once per
process; with 0 it keeps the thread-per-segment walk k_hash_bwd_ray<4>, <8> instead of the lane-per-feature k_hash_bwd_ray_fl.  Runs that walk on lmf-L3-F4 and lmf-L16-F8 at
(701, 37) against the exact sum, under the float paths' bound.  Exit status 0 = both within the bound."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

assert os.environ.get("NRF_HASH_BWD_FEATURE_LANES") == "0", "start me with NRF_HASH_BWD_FEATURE_LANES=0"

import torch  # noqa: E402

import hash_backward_paths as G  # noqa: E402
import hash_backward_ref as B  # noqa: E402
from nerfpp_amd import _lib as L, modules as M  # noqa: E402


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    n, s = B.MAIN
    for name in ("lmf-L3-F4", "lmf-L16-F8"):
        case = B.BY_NAME[name]
        i, ex = B.inputs(name, n, s), B.expected_exact(name, n, s)
        got = G.run_float(L, G.make_handle(M, case), "rays", i, n, s)
        G.check_against_exact(got, i, ex, G.float_tolerance(i, ex), f"{name} thread-per-segment walk")
    print("ok")


if __name__ == "__main__":
    main()
