"""CPU tests (no GPU): the C-ABI library loads and exports every declared symbol, host-side logic (synthetic scenes,
row-tile sharding, argument validation that happens before any device call), and the 2-rank gloo path of the
multi-GPU gather."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from nerfpp_amd import synth


def test_library_builds_loads_and_exports_every_header_symbol():
    import __graft_entry__ as g
    from nerfpp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "nerfpp_hip.h")).read()
    declared = set(re.findall(r"NRF_API\s+[\w\s\*]+?\b(nrf_\w+)\s*\(", hdr))
    assert len(declared) >= 35
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    for s in declared:
        assert hasattr(lib, s), f"libnerfpp_hip.so does not export {s}"
    lib.nrf_status_string.restype = C.c_char_p
    assert lib.nrf_status_string(0) == b"ok" and lib.nrf_version() >= 100


def test_signature_table_matches_the_header_for_every_entry_point():
    """_lib.SIGNATURES is the only place the Python side states the C ABI: every NRF_API declaration of the header, parsed
    here independently, must give the same name, argument count, argument kinds and return kind, and the loaded library
    must carry exactly those argtypes / restype.  No function is exempt."""
    from nerfpp_amd import _lib
    scalars = {"int": "i", "int64_t": "l", "size_t": "z", "float": "f", "double": "d", "uint32_t": "u", "uint64_t": "q"}
    ctype = {"i": C.c_int, "l": C.c_int64, "z": C.c_size_t, "f": C.c_float, "d": C.c_double, "u": C.c_uint32, "q": C.c_uint64,
             "p": C.c_void_p, "s": C.c_char_p, "v": None}

    def kind(decl, fn, named):
        if "*" in decl or "[" in decl:
            return "p"
        words = [w for w in decl.split() if w != "const"]
        typ = " ".join(words[:-1] if named and len(words) > 1 else words)
        assert typ in scalars, f"{fn}: no kind for `{decl.strip()}`"
        return scalars[typ]

    hdr = open(os.path.join(ROOT, "include", "nerfpp_hip.h")).read()
    hdr = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))
    decls = re.findall(r"\bNRF_API\s+([\w\s\*]+?)\b(nrf_\w+)\s*\(([^()]*)\)\s*;", hdr)
    uses = sum(len(re.findall(r"\bNRF_API\b", line)) for line in hdr.splitlines() if not line.lstrip().startswith("#"))
    assert len(decls) == uses >= 194, f"the regex parsed {len(decls)} of the header's {uses} NRF_API declarations"
    header = {}
    for ret, fn, args in decls:
        ret = " ".join(ret.replace("*", " * ").split())
        r = {"void": "v", "const char *": "s"}.get(ret) or kind(ret, fn, named=False)
        a = "" if args.strip() in ("", "void") else "".join(kind(x, fn, named=True) for x in args.split(","))
        assert fn not in header, f"{fn} is declared twice"
        header[fn] = (r, a)
    assert set(header) == set(_lib.SIGNATURES) == set(_lib.SYMBOLS), set(header) ^ set(_lib.SIGNATURES)
    assert list(header) == _lib.SYMBOLS, "the table is kept in the header's order"
    wrong = {fn: (_lib.SIGNATURES[fn], sig) for fn, sig in header.items() if _lib.SIGNATURES[fn] != sig}
    assert not wrong, f"(table, header) differ for {wrong}"
    lib = _lib.lib()
    for fn, (r, a) in header.items():
        f = getattr(lib, fn)
        assert f.restype is ctype[r] and f.argtypes is not None and list(f.argtypes) == [ctype[k] for k in a], fn
    with pytest.raises(TypeError):
        lib.nrf_pe_encode(None, 4, 10, None)             # one argument short: refused before the call
    with pytest.raises(C.ArgumentError):
        lib.nrf_pe_encode(None, 4.0, 10, None, None)     # a float where the header says int64_t


def test_argument_validation_needs_no_gpu():
    from nerfpp_amd import _lib
    lib = _lib.lib()
    assert lib.nrf_pe_encode(None, C.c_int64(4), 10, None, None) == 1          # NRF_ERR_INVALID_ARG
    assert b"nrf_pe_encode" in lib.nrf_last_error()
    d = _lib.HashDesc(7, 16, 2, 19, 16, 512, (C.c_float * 6)(-1, -1, -1, 1, 1, 1))
    h = C.c_void_p()
    assert lib.nrf_hash_create(C.byref(d), C.byref(h)) == 1 and b"unknown mode" in lib.nrf_last_error()
    d.mode = 0; d.n_features = 3
    assert lib.nrf_hash_create(C.byref(d), C.byref(h)) == 1
    out = np.empty(64, np.float32)
    assert lib.nrf_linspace(C.c_float(0), C.c_float(1), 64, out.ctypes.data_as(C.c_void_p)) == 0
    assert (out == load_golden("sample_pdf")["aux_t64"]).all()                  # host helper == ATen bit for bit
    sd = _lib.MlpSmallDesc(32, 16, 3, 64, 15, 4, 64)
    assert lib.nrf_mlp_small_param_count(C.byref(sd)) == 17536                 # 17 536 MAC / point
    nd = _lib.MlpNerfDesc(8, 256, 63, 27, 4, 4, 1)
    assert lib.nrf_mlp_nerf_param_count(C.byref(nd)) == 593408 + 8 * 256 + 128 + 256 + 1 + 3   # 593 408 weights + biases


def test_no_cpu_fallback_without_device():
    """On a box without a GPU the compute entry points must FAIL (NRF_ERR_HIP), never compute on the host."""
    if torch.cuda.is_available():
        pytest.skip("has a GPU")
    from nerfpp_amd import _lib
    lib = _lib.lib()
    d = _lib.HashDesc(0, 4, 2, 10, 4, 32, (C.c_float * 6)(-1, -1, -1, 1, 1, 1))
    h = C.c_void_p()
    assert lib.nrf_hash_create(C.byref(d), C.byref(h)) == 2                     # NRF_ERR_HIP: hipMalloc fails
    assert b"hipMalloc" in lib.nrf_last_error()


def test_scene_synth_reproduces_golden_manifest(manifest):
    from nerfpp_amd import scene
    ent = manifest["render_hash"]
    mlp = [e for e in ent if "embeddings" not in e[0]]
    mine = scene.synth_linear_stack(scene.small_shapes(), 6000, 1.6, 0.0, {"sigma_net_2": 30.0})
    ref = synth.params_from_manifest(mlp)
    assert [n for n, _ in mine] == [n for n, _ in ref]
    for (_, a), (_, b) in zip(mine, ref):
        assert a.shape == b.shape and (a == b).all()
    table = scene.synth_hash_table(16, 19, 2, 5000, 0.5)
    assert (table[:1024] == synth.blob_from_manifest(ent[:1])[:1024]).all()
    cl = scene.synth_linear_stack(scene.nerf_shapes(), 7000, 1.4, 0.1, {"alpha_linear.weight": 40.0})
    ref = synth.params_from_manifest(manifest["render_classic"])
    assert [n for n, _ in cl] == [n for n, _ in ref]
    assert all((a == b).all() for (_, a), (_, b) in zip(cl, ref))


def test_pose_spherical_and_camera():
    from nerfpp_amd import scene
    c2w = scene.pose_spherical(30.0, -30.0, 4.0)
    assert c2w.shape == (3, 4)
    assert abs(np.linalg.norm(c2w[:, 3]) - 4.0) < 1e-5                           # camera on the radius-4 sphere
    assert np.allclose(c2w[:, :3] @ c2w[:, :3].T, np.eye(3), atol=1e-6)          # rotation
    fwd = -c2w[:, 2]                                                             # looks at the origin
    assert np.allclose(fwd, -c2w[:, 3] / 4.0, atol=1e-5)
    K = scene.lego_K(800, 800)
    assert abs(K[0, 0] - 1111.111) < 1e-2 and K[0, 2] == 400
    assert abs(scene.lego_K(400, 400)[0, 0] - 555.5555) < 1e-2
    assert len(set(scene.CU_PRIMES)) == 96 and all((1 << 28) <= p < (1 << 30) for p in scene.CU_PRIMES)
    assert all(all(p % q for q in range(2, int(p ** 0.5) + 1)) for p in scene.CU_PRIMES[:6])


def test_tile_shard_partition():
    from nerfpp_amd.dist import TileShard
    for h, n in ((800, 1), (800, 2), (800, 8), (10, 4), (7, 3)):
        shards = [TileShard(h, 5, r, n) for r in range(n)]
        assert sum(s.rows for s in shards) == h
        assert [s.row0 for s in shards] == [sum(s2.rows for s2 in shards[:i]) for i in range(n)]
    s = TileShard(6, 4)
    t = torch.arange(6 * 4 * 3, dtype=torch.float32).reshape(6, 4, 3)
    assert torch.equal(s.all_gather_frames([t, t + 1])[1], t + 1)


def test_tile_partition_c_abi():
    """nrf_tile_partition: the tile bookkeeping of the C++ / LibTorch host (HipNeRFRenderer::RenderSharded) -- contiguous, covering, balanced to one row."""
    from nerfpp_amd import _lib
    from nerfpp_amd.dist import tile_partition
    for h, n in ((800, 1), (800, 2), (800, 3), (800, 7), (800, 8), (10, 4), (7, 3), (3, 8), (0, 2)):
        parts = [tile_partition(h, n, r) for r in range(n)]
        assert parts[0][0] == 0 and sum(p[1] for p in parts) == h
        assert all(parts[r + 1][0] == parts[r][0] + parts[r][1] for r in range(n - 1))
        assert max(p[1] for p in parts) - min(p[1] for p in parts) <= 1
    assert tile_partition(800, 8, 3) == (300, 100)            # 800 / 8 = 100 rows = 80 000 rays per rank
    r0, rr = C.c_int(), C.c_int()
    lib = _lib.lib()
    assert lib.nrf_tile_partition(800, 8, 8, C.byref(r0), C.byref(rr)) == 1 and b"rank" in lib.nrf_last_error()
    assert lib.nrf_tile_partition(800, 0, 0, C.byref(r0), C.byref(rr)) == 1
    assert lib.nrf_allgather_tiles(None, None, 1, 8, 8, 3, None, None) == 1 and b"communicator" in lib.nrf_last_error()


def test_render_view_dims_vs_reference():
    """The render-factor step of NeRFExecutor::RenderView (NeRFExecutor.h:618-627) against the golden from its own statements."""
    from nerfpp_amd import _lib
    g = load_golden("render_factor")
    h, w = (int(v) for v in g["hw"])
    K = np.ascontiguousarray(g["k"], np.float32)
    K1 = np.empty(9, np.float32)
    h1, w1 = C.c_int(), C.c_int()
    lib = _lib.lib()
    assert lib.nrf_render_view_dims(h, w, K.ctypes.data_as(C.c_void_p), C.c_float(float(g["render_factor"][0])), C.byref(h1), C.byref(w1), K1.ctypes.data_as(C.c_void_p)) == 0
    assert [h1.value, w1.value] == list(g["aux_hw1"]) == [8, 8]
    assert (K1.reshape(3, 3) == g["aux_k1"]).all()
    assert lib.nrf_render_view_dims(h, w, K.ctypes.data_as(C.c_void_p), C.c_float(0.0), C.byref(h1), C.byref(w1), K1.ctypes.data_as(C.c_void_p)) == 0
    assert (h1.value, w1.value) == (h, w) and (K1 == K.reshape(-1)).all()       # RenderFactor == 0: untouched
    assert lib.nrf_render_view_dims(h, w, K.ctypes.data_as(C.c_void_p), C.c_float(2.0), C.byref(h1), C.byref(w1), None) == 0 and h1.value == 13   # RenderPath's use: dims only


GLOO_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ["NRF_ROOT"])
from nerfpp_amd.dist import TileShard
rank = int(os.environ["RANK"]); world = int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
H, W, F = 7, 5, 3                       # uneven split: 4 + 3 rows
full = torch.arange(F * H * W * 3, dtype=torch.float32).reshape(F, H, W, 3)
sh = TileShard(H, W, rank, world)
tiles = [full[f, sh.row0:sh.row0 + sh.rows].clone() for f in range(F)]
out = sh.all_gather_frames(tiles)
assert out.shape == full.shape and torch.equal(out, full), "gathered frames differ"
dist.barrier()
t = torch.tensor([float(rank + 1)], dtype=torch.float64)
dist.all_reduce(t, op=dist.ReduceOp.MAX)
assert t.item() == world
# data-parallel gradient mean (GradSync): bucketed all-reduce, in place, uneven last bucket
from nerfpp_amd.dist import GradSync
g_table = torch.arange(1000, dtype=torch.float32) * (rank + 1); g_blob = torch.full((7,), float(rank), dtype=torch.float32)
GradSync(bucket_bytes=4 * 300)(g_table, g_blob)
assert torch.allclose(g_table, torch.arange(1000, dtype=torch.float32) * (sum(range(1, world + 1)) / world)) and torch.allclose(g_blob, torch.full((7,), (world - 1) / 2.0))
# one frame, equal tiles: the gathered buffer is the frame itself (the strong-scaling step of bench.py)
H2 = 8
full2 = torch.arange(H2 * W * 3, dtype=torch.float32).reshape(1, H2, W, 3)
sh2 = TileShard(H2, W, rank, world)
out2 = sh2.all_gather_frames([full2[0, sh2.row0:sh2.row0 + sh2.rows].clone()])
assert out2.shape == full2.shape and torch.equal(out2, full2)
# ... issued asynchronously (bench.py's step: the next frame's render is not held behind the collective); the frame may be read after work.wait()
out3, work = sh2.all_gather_frames([full2[0, sh2.row0:sh2.row0 + sh2.rows].clone()], overlap=True)
assert work is not None
work.wait()
assert torch.equal(out3, full2)
out4, work4 = sh.all_gather_frames(tiles, overlap=True)          # uneven tiles: re-assembled behind the collective, nothing pending
assert work4 is None and torch.equal(out4, full)
# the fp16 backward's overflow flag is per rank; the decision to skip the optimizer step is collective and comes BEFORE any gradient is exchanged
gs = GradSync()
g1 = torch.ones(10); g2 = torch.ones(3)
if rank == 1:
    g1[4] = float("inf")
skip = gs.reduce_or_skip(rank == 1, g1, g2)
assert skip is True, "every rank skips when any rank overflowed"
assert torch.isfinite(g1).all() == (rank == 0) and torch.equal(g2, torch.ones(3)), "no gradient was summed: rank 0 keeps its finite one, the inf stays where it arose"
skip = gs.reduce_or_skip(False, g2)
assert skip is False and torch.equal(g2, torch.ones(3))
dist.destroy_process_group()
print("ok", rank)
"""


def test_tile_all_gather_two_ranks_gloo(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(GLOO_WORKER)
    env = dict(os.environ, NRF_ROOT=ROOT, MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", "29533", str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("ok") == 2


# ------------------------------------------------------------------ N3: checkpoint interchange with the reference
def test_read_reference_checkpoints(manifest):
    """tests/golden/ckpt/*.pt were written by the reference's own torch::save calls (oracle/_ref/ref_driver ckpt_save, NeRFExecutor.h:1058-1066)."""
    from nerfpp_amd import checkpoint as CK, synth
    d = os.path.join(ROOT, "tests", "golden", "ckpt")
    ck = CK.LoadCheckpoint(d)
    assert ck["start"] == 1234
    assert list(ck["model"].keys()) == [f"model_{n}.weight" for n in ("sigma_net_0", "sigma_net_1", "sigma_net_2", "color_net_0", "color_net_1", "color_net_2")]
    ent = manifest["train_hash"]          # ckpt_save fills the modules with the train_hash seeds
    np.testing.assert_array_equal(CK.blob(ck["model"]), synth.blob_from_manifest([e for e in ent if "embeddings" not in e[0]]))
    np.testing.assert_array_equal(CK.blob(ck["embedder"]), synth.blob_from_manifest([e for e in ent if "embeddings" in e[0]]))
    p, b = CK.load_module(os.path.join(d, "cu_embedder_checkpoint.pt"))
    table, primes, biases = CK.cu_hash_state(p, b)
    assert table.shape == (4 * 4096, 2) and primes.shape == (12,) and primes[0] == 268435459 and primes[5] == 268435469 and (biases == 0.25).all()
    assert list(b["embedder_feat_local_idx"]) == [0, 4096, 8192, 12288]
    # the reference's own torch::save(*Optimizer) (NeRFExecutor.h:1067): Adam(lr 5e-4, betas (0.9, 0.99), eps 1e-15) after one step
    assert ck["would_restore"]
    opt = ck["optimizer"]
    assert opt["step"] == 1 and abs(opt["lr"] - 5e-4) < 1e-12 and opt["betas"] == (0.9, 0.99) and opt["eps"] == 1e-15 and len(opt["moments"]) == 10
    g0 = synth.synth_sym(9000, (4096, 2), np.float32(1e-2))               # the driver's synthetic gradient of parameter 0: after one step m = 0.1 g, v = 0.01 g^2
    np.testing.assert_allclose(opt["moments"][0][0], np.float32(0.1) * g0, rtol=1e-6)
    np.testing.assert_allclose(opt["moments"][0][1], np.float32(0.01) * g0 * g0, rtol=2e-6)


CKPT_WRITTEN_SHA256 = os.path.join(ROOT, "tests", "golden", "ckpt_written.sha256")


def written_checkpoint_inputs():
    """The seeded model / embedder / Adam state / CuHashEmbedder state of test_written_checkpoints_restore_a_reference_model (also oracle/make_golden.py)."""
    rng = np.random.RandomState(4)
    model = {f"model_{n}.weight": rng.randn(*s).astype(np.float32) for n, s in (("sigma_net_0", (64, 8)), ("sigma_net_1", (64, 64)), ("sigma_net_2", (16, 64)),
                                                                              ("color_net_0", (64, 31)), ("color_net_1", (64, 64)), ("color_net_2", (3, 64)))}
    emb = {f"embedder_embeddings_{l}.weight": rng.randn(4096, 2).astype(np.float32) for l in range(4)}
    # Adam state in the optimizer's parameter order (NeRFExecutor.h:508-535: the embedder's parameters, then the model's)
    shapes = [v.shape for v in emb.values()] + [v.shape for v in model.values()]
    mom = [(rng.randn(*s_).astype(np.float32), rng.rand(*s_).astype(np.float32)) for s_ in shapes]
    mom[2] = None                                                      # a parameter that has not been stepped yet has no state
    cu_p = {"embedder_embeddings": rng.randn(4 * 4096, 2).astype(np.float32)}
    cu_b = {"embedder_primes": (268435459 + np.arange(12, dtype=np.int32) * 4).reshape(4, 1, 3), "embedder_biases": np.full((4, 3), 0.5, np.float32),
            "embedder_feat_local_size": np.full(4, 4096, np.int32), "embedder_feat_local_idx": (np.arange(4) * 4096).astype(np.int32)}
    return model, emb, mom, cu_p, cu_b


def write_checkpoint_in_fresh_process(d):
    """SaveCheckpoint + the CuHashEmbedder archive of written_checkpoint_inputs() into `d`, in a child process: TorchScript numbers the classes it
    compiles per process (___torch_mangle_<n>), so only a fresh process writes the same bytes every time."""
    code = ("import sys; sys.path[:0] = [sys.argv[1], sys.argv[2]]\n"
            "from test_host_cpu import written_checkpoint_inputs\n"
            "from nerfpp_amd import checkpoint as CK\n"
            "model, emb, mom, cu_p, cu_b = written_checkpoint_inputs()\n"
            "CK.SaveCheckpoint(sys.argv[3], embedder=emb, model=model, global_step=77, optimizer=dict(moments=mom, step=41, lr=3e-4))\n"
            "CK.save_module(sys.argv[3] + '/cu_embedder_checkpoint.pt', cu_p, cu_b)\n")
    subprocess.check_call([sys.executable, "-c", code, ROOT, os.path.join(ROOT, "tests"), d])


def checkpoint_sha256(d):
    """Per archive in `d`: SHA-256 over its members (name, bytes) except the debug tables (*.debug_pkl: source ranges, with the absolute path of the writing
    checkout) and .data/serialization_id (derived from them) -- code, pickles and tensor data, what torch::load reads."""
    import hashlib
    import zipfile
    out = {}
    for f in sorted(os.listdir(d)):
        if not f.endswith(".pt"):
            continue
        h = hashlib.sha256()
        with zipfile.ZipFile(os.path.join(d, f)) as z:
            for n in z.namelist():
                if n.endswith(".debug_pkl") or n.endswith("/.data/serialization_id"):
                    continue
                h.update(n.encode() + b"\0" + z.read(n))
        out[f] = h.hexdigest()
    return out


def test_written_checkpoints_restore_a_reference_model(tmp_path):
    """SaveCheckpoint -> the reference's torch::load into ITS HashEmbedder / NeRFSmall (oracle/_ref/ref_driver ckpt_load) -> same numbers.  Where ref_driver is
    not built, the archives must hold byte for byte what it restored when tests/golden/ckpt_written.sha256 was recorded (oracle/make_golden.py); where it
    is, both hold."""
    from nerfpp_amd import checkpoint as CK
    model, emb, mom, cu_p, cu_b = written_checkpoint_inputs()
    d = str(tmp_path / "ck"); out = str(tmp_path / "out"); os.makedirs(out)
    assert not CK.WouldRestore(str(tmp_path))
    write_checkpoint_in_fresh_process(d)
    assert CK.WouldRestore(d)                                           # the reference's own condition (NeRFExecutor.h:541-546): start + optimizer + model files
    want = dict(line.split()[::-1] for line in open(CKPT_WRITTEN_SHA256) if line.strip())
    assert checkpoint_sha256(d) == want, "the archives differ from the ones the reference restored (re-record with oracle/make_golden.py where ref_driver is built)"
    back = CK.LoadCheckpoint(d)
    assert back["would_restore"] and back["optimizer"]["step"] == 41 and back["optimizer"]["moments"][2] is None
    np.testing.assert_array_equal(back["optimizer"]["moments"][5][1], mom[5][1])
    for k, v in model.items():
        np.testing.assert_array_equal(back["model"][k], v)
    for k, v in emb.items():
        np.testing.assert_array_equal(back["embedder"][k], v)
    drv = os.path.join(ROOT, "oracle", "_ref", "ref_driver")
    if not os.path.exists(drv):
        return
    subprocess.check_call([drv, "ckpt_load", d, out], stdout=subprocess.DEVNULL)
    for k, v in model.items():
        np.testing.assert_array_equal(np.load(os.path.join(out, "m." + k + ".npy")), v)
    for k, v in emb.items():
        np.testing.assert_array_equal(np.load(os.path.join(out, "e." + k + ".npy")), v)
    np.testing.assert_array_equal(np.load(os.path.join(out, "cu.embedder_embeddings.npy")), cu_p["embedder_embeddings"])
    np.testing.assert_array_equal(np.load(os.path.join(out, "cu.embedder_primes.npy")), cu_b["embedder_primes"])
    assert int(np.load(os.path.join(out, "start.npy"))[0]) == 77
    # torch::load(*Optimizer, "optimizer_checkpoint.pt") (:565) into the reference's Adam: moments, step and lr arrive value for value
    assert int(np.load(os.path.join(out, "opt.would_restore.npy"))[0]) == 1
    assert np.load(os.path.join(out, "opt.lr.npy"))[0] == np.float32(3e-4)
    for i, mv in enumerate(mom):
        f = os.path.join(out, f"opt.{i}.exp_avg.npy")
        if mv is None:
            assert not os.path.exists(f)
            continue
        np.testing.assert_array_equal(np.load(f), mv[0])
        np.testing.assert_array_equal(np.load(os.path.join(out, f"opt.{i}.exp_avg_sq.npy")), mv[1])
        assert np.load(os.path.join(out, f"opt.{i}.step.npy"))[0] == 41


def test_bench_launcher_reports_failing_ranks_without_hanging():
    """`python bench.py --gpus 2` with no launcher: the parent starts the ranks itself and must return non-zero -- promptly -- when a rank fails
    (here rank 1 exits at start-up through the test hook; on a box without a GPU rank 0 fails too, at its "needs MI355X" assertion)."""
    import time
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "1", "--warmup", "0", "--no-cpu-baseline",
                        "--no-also", "--no-parity"], capture_output=True, text=True, timeout=300, env=dict(os.environ, NRF_BENCH_TEST_FAIL_RANK="1", NRF_BENCH_TIMEOUT="120"))
    assert r.returncode != 0 and "rank exit codes" in r.stderr, (r.returncode, r.stderr[-500:])
    assert time.time() - t0 < 200
    assert not [x for x in r.stdout.splitlines() if x.startswith("{")], "no result line from a failed run"
    # contradictory flags are rejected by the parent before anything is started
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--collective", "cabi"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "cabi" in r.stderr


def test_bench_full_option_is_off_by_default():
    """A plain `bench.py` run times the headline only; every other measurement and check is behind --full (argparse answers --help before any GPU API is touched)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--full" in r.stdout, r.stderr[-500:]
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert 'ap.add_argument("--full", action="store_true"' in src, "off unless asked for"


def _canned_bench_detail(world):
    """A full bench record assembled from canned measurements (round 3's HIP-event totals) through the same functions bench.py calls on the GPU box."""
    from benchlib import roofline as RF
    from benchlib.costs import H, W, UNITS_PER_RAY
    timed = {"hash": dict(ms=156.26, launches=120), "mlp": dict(ms=89.19, launches=60), "composite": dict(ms=59.88, launches=120), "sample": dict(ms=27.05, launches=60),
             "other": dict(ms=0.0, launches=0), "sigma": dict(ms=56.47, launches=60), "mlp_colour": dict(ms=42.46, launches=60)}
    single = {"hash": dict(ms=36.64, launches=50), "mlp": dict(ms=34.70, launches=25), "composite": dict(ms=9.1, launches=50), "sample": dict(ms=4.4, launches=25),
              "other": dict(ms=0.0, launches=0), "sigma": dict(ms=24.47, launches=25), "mlp_colour": dict(ms=10.94, launches=25)}
    units = H * W * UNITS_PER_RAY / world
    roof = dict(timed=RF.kernel_rooflines(timed, "hash", "f16x3", "cu", units * 10), lanes_timed=2, kernel_ms_timed=timed, profile_events_in_timed_region=False,
                lanes=dict(requested="auto", chosen=2, ms_per_step_by_lanes={"1": 23.435, "2": 22.003}))
    if world == 1:
        roof["isolated"] = RF.kernel_rooflines(single, "hash", "f16x3", "cu", units * 5)
        roof["isolated_kernel_sum_ms_per_step"] = sum(v["ms"] for v in single.values()) / 5
    long_text = "x" * 1500          # prose that once rode in the line (traffic_source, notes): must not reach it again
    also = [dict(workload="hashnerf_lego800_64+128", baseline_config=3, precision="f16", value=12179889925.4, unit="ray-samples/s", ms_per_step=13.45, steps=10,
                 kernel_ms=timed, roofline=dict(frac=0.3964, note=long_text), psnr_vs_oracle_db=dict(psnr=44.08, max_abs_err=0.116)),
            dict(workload="classic_nerf_lego800_64+128", precision="f16x3", value=3.18e8, ms_per_step=514.4, coarse_pass="density branch in exact fp32 " + long_text,
                 roofline=dict(frac=0.2086), psnr_vs_oracle_db=dict(psnr=141.16)),
            dict(workload="classic_nerf_lego800_64+128", precision="f16x3", value=5.61e8, ms_per_step=291.9, coarse_pass="whole network in the timed arithmetic",
                 roofline=dict(frac=0.2039), psnr_vs_oracle_db=dict(psnr=118.33)),
            dict(workload="classic_nerf_lego800_64+128", precision="f16", value=1.5e9, ms_per_step=108.1, roofline=dict(frac=0.5653), psnr_vs_oracle_db=dict(psnr=58.4)),
            dict(workload="hashnerf_lego800_64+128", encoder="HashEmbedder + SHEncoder (LibTorch twin)", precision="f16x3", value=5.83e9, ms_per_step=28.1,
                 psnr_vs_oracle_db=dict(psnr=138.95)),
            dict(workload="hashnerf_train_step", value=4.5e8, ms_per_step=9.31, arithmetic=long_text, cpu_reference=dict(sample=long_text)),
            dict(workload="lerf_lego800_64+128", precision="f16x3", value=1.12e9, s_per_frame=0.1458, arithmetic=long_text, roofline=dict(frac=0.2857),
                 oracle_check=dict(embedding_cos_min=0.99999988, fine_sample_set_bit_identical_rays=1.0)),
            dict(workload="lerf_lego800_64+128", precision="f16", value=1.58e9, s_per_frame=0.1038, roofline=dict(frac=0.4867),
                 oracle_check=dict(embedding_cos_min=0.99174, fine_sample_set_bit_identical_rays=0.0)),
            dict(workload="lerf_lego800_64+128", error=long_text)]
    # the C++ / LibTorch host's own lines (benchlib/extras.py::dropin_measurements: oracle/_ref/adapter_check bench)
    also += [dict(workload="dropin_" + w, precision="f16x3", value=v, unit="ray-samples/s", ms_per_step=ms, host="C++ / LibTorch (adapter_check bench)", detail=dict(note=long_text))
             for w, v, ms in (("frame_hash", 7.5e9, 21.83), ("frame_classic", 3.2e8, 508.4), ("frame_lerf", 1.24e9, 132.0), ("train_hash", 6.8e8, 6.14),
                              ("train_hash_hipadam", 7.2e8, 5.81), ("train_classic", 2.05e7, 51.0), ("train_lerf", 7.3e7, 57.1))]
    if world > 1:
        also = [dict(scaling="weak", frames_per_step=world, steps=5, ms_per_step=23.0, value=7.1e9 * world, unit="ray-samples/s", host_ms_per_tile=0.4, finite=True)]
    return {"metric": "ray-samples/sec (HIP volume-rendering path, Lego 800x800, N_samples=64+128)", "value": 7302017868.09 * world, "unit": "ray-samples/s",
            "n_gpus": world, "steps": 10, "warmup": 2, "ms_per_step": 22.4376 / world, "higher_is_better": True, "scaling": "weak" if world == 1 else "strong",
            "vs_baseline": None, "dtype": "f16x3", "data": "synthetic",
            "config": {"workload": "hashnerf_lego800_64+128", "baseline_config": 3, "encoder": "CuHashEmbedder L16 T2^19 F2 16..512 + CuSHEncoder deg4 + NeRFSmall 3x64/4x64",
                       "oracle_pin": "restatement (CUDA-only encoders; reference-pinned twin in also)", "frames_per_step": 1, "rays_per_gpu_per_step": 640000 // world,
                       "ray_samples_per_ray": 256, "chunk": 131072,
                       "parallelism": f"row-tile x{world}" + (" + RCCL all_gather (torch.distributed)" if world > 1 else "")},
            "executed_evaluations_per_ray": dict(hash_encode=192, fused_mlp=128, sigma_only=64, colour_net_only=64),
            "rays_per_s": 28523507.3 * world, "s_per_frame": 0.0224 / world, "host_ms_per_tile": 0.4066, "tile_rows": 800 // world, "roofline": roof,
            "ranks_seen_by_rccl": world if world > 1 else None, "collective": "nrf_allgather_tiles (C ABI)" if world > 1 else None, "host_ms_per_tile_mean": 5.25,
            "collective_check": ("nrf_allgather_tiles (C ABI, RCCL) == torch.distributed all_gather_into_tensor on every rank " + long_text) if world > 1 else None,
            "cpu_baseline": dict(value=418719.8, unit="ray-samples/s", cores=256, threads=32, kind="reference", thread_sweep={"8": 364710}, host_cpus=256, sample="18400 rays " + long_text),
            "psnr_vs_oracle_db": dict(psnr=140.55, max_abs_err=7.2e-7), "parity_full_frame_vs_f32": dict(pixels=640000, max_abs_err=2.74e-6, psnr=140.06),
            "frame_sha256": "dcaf99dc2ffe33542a3dbbdcf2b0fbcaf4ab6a2b313c8cd326bc029bcab65afb", "also": also}


@pytest.mark.parametrize("world", [1, 2, 8])
def test_bench_result_line_is_compact_complete_and_parseable(world, tmp_path, capsys):
    """The one JSON line the driver parses (round 3's grew to 29 KB and was lost: BENCH_r03.json.parsed = null): < 4 KB for the --gpus 1 and the --gpus N
    shapes, round-trips through json, carries every key of the driver's contract plus a flat `roofline` and `cpu_baseline`; the top-level roofline is the
    dominant kernel of the SINGLE-LANE pass and re-derives from its own fields; everything else lands in the side file."""
    import json
    from benchlib import report
    detail = _canned_bench_detail(world)
    report.emit(detail, stats_csv="profiles/round6/r8m_single_lane_kernel_stats.csv", path=str(tmp_path / "bench_detail.json"))
    cap = capsys.readouterr()
    out_lines = cap.out.strip().splitlines()
    assert len(out_lines) == 1, "ONE line on stdout"
    s = out_lines[0]
    assert len(s) < report.LINE_LIMIT == 4096, len(s)
    line = json.loads(s)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline",
              "cpu_baseline", "psnr_vs_oracle_db", "frame_sha256"):
        assert k in line, k
    assert set(line["config"]) >= {"workload", "baseline_config", "encoder", "frames_per_step", "rays_per_gpu_per_step", "chunk", "parallelism"} and "model" not in line["config"]
    assert line["n_gpus"] == world and line["scaling"] == ("weak" if world == 1 else "strong") and line["vs_baseline"] is None and line["dtype"] == "f16x3"
    assert set(line["cpu_baseline"]) == {"value", "unit", "cores", "threads", "kind", "sample"} and len(line["cpu_baseline"]["sample"]) <= 160
    assert line["cpu_baseline"]["cores"] == 256 and line["cpu_baseline"]["threads"] == 32            # cores: the box's; threads: the count that won the sweep
    assert line["profile_events_in_timed_region"] is False and line["lanes_timed"] == 2 and line["ms_per_step_by_lanes"] == {"1": 23.435, "2": 22.003}
    assert line["config"]["baseline_config"] == 3                                                     # 1-based: config 3 = HashNeRF 800x800 on one GPU
    r = line["roofline"]
    assert {"bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "launches", "avg_launch_ms", "units_per_launch"} <= set(r)
    assert r["bound"] in ("hbm", "mfma") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    if world == 1:
        # the isolated (single-lane) dominant kernel: NeRFSmall on the matrix cores; units x flop / launch time re-derives `achieved` (TFLOP/s)
        assert r["lanes"] == 1 and r["kernel"].startswith("mlp_small") and r["bound"] == "mfma" and r["kernel_stats"].startswith("profiles/round6/")
        assert abs(r["units_per_launch"] * r["flop_per_unit"] / (r["avg_launch_ms"] * 1e-3) / 1e12 - r["achieved"]) < 0.01 * r["achieved"]
        assert 0.1 < r["frac"] < 0.25 and 0.4 < r["mfma_issued_frac"] < 0.8
        # hash: no fraction above 1 any more -- frac is the COUNTER fraction of the HBM peak (absent while the kernel's sources differ from the profiled ones),
        # the gathered bytes are priced against the cache-resident gather ceiling
        assert r["hash"]["unit"] == "GB/s" and r["hash"].get("frac", 0.0) < 1.0 and 0.5 < r["hash"]["gather_frac_of_cache_ceiling"] < 1.5 and r["sigma"]["frac"] < 1.0
        assert abs(r["kernel_sum_ms_per_step"] - 24.05) < 0.01
        assert len(line["also"]) == 16 and all(len(json.dumps(a)) <= 140 for a in line["also"])
        assert [a["workload"] for a in line["also"]][9:] == ["dropin_frame_hash", "dropin_frame_classic", "dropin_frame_lerf", "dropin_train_hash", "dropin_train_hash_hipadam",
                                                             "dropin_train_classic", "dropin_train_lerf"] and line["also"][9]["ms"] == 21.83
        assert [a["workload"] for a in line["also"]][:5] == ["hashnerf", "classic_nerf", "classic_nerf_coarse_full", "classic_nerf", "hashnerf_libtorch_twin"]
    else:
        assert r["lanes"] == 2 and line["ranks_seen_by_rccl"] == world and len(line["collective_check"]) <= 100 and line["also"][0]["workload"] == "scaling_weak"
        assert line["collective"].startswith("nrf_allgather_tiles")
    assert "x" * 200 not in s, "prose stays in the side file"
    side = json.load(open(tmp_path / "bench_detail.json"))
    assert side["roofline"]["timed"]["hash"]["launches"] == 120 and side["also"] and "[bench detail] {" in cap.err
    # a record that would still be too large loses its optional parts, never the headline
    detail["also"] = [dict(workload="w%d" % i, precision="f16x3", value=1.0, ms_per_step=1.0, psnr_vs_oracle_db=dict(psnr=100.0), roofline=dict(frac=0.5)) for i in range(80)]
    s2 = report.dumps_line(report.compact_line(detail))
    l2 = json.loads(s2)
    assert len(s2) < 4096 and "also" not in l2 and l2["dropped_for_size"] == ["also: workload + ms only", "also"] and l2["value"] == line["value"] and "cpu_baseline" in l2
    # ... and a moderately oversized one keeps its entries, shortened
    detail["also"] = [dict(workload="w%d" % i, precision="f16x3", value=123456789.0, ms_per_step=1.0, psnr_vs_oracle_db=dict(psnr=100.0), roofline=dict(frac=0.5)) for i in range(38)]
    l3 = json.loads(report.dumps_line(report.compact_line(detail)))
    assert len(l3["also"]) == 38 and set(l3["also"][0]) == {"workload", "ms"} and l3["dropped_for_size"] == ["also: workload + ms only"]


def test_timed_region_refuses_to_run_with_the_per_kernel_event_bracketing_on():
    """bench.py's headline is timed by benchlib/timing.py's timed_region, which asserts nrf_profile_is_enabled() == 0 before and after the K steps: round 4's driver-measured
    30.1 ms per frame carried two timing events around every kernel of both lanes (the claimed 22 ms did not).  With the real library (loads without a GPU; the flag is host
    state) the region runs with the bracketing off and raises with it on; bench.py's own timed path goes through it and no longer has a profile= switch."""
    import re
    from benchlib import timing
    from nerfpp_amd import _lib as L
    lib = L.lib()
    assert lib.nrf_profile_is_enabled() == 0, "off by default"
    calls = []
    dt, out = timing.timed_region(lib, lambda: calls.append(1) or len(calls), lambda: calls.append("drain"), lambda: calls.append("sync"), 4)
    assert calls == ["sync", 1, 1, 1, 1, "drain", "sync"] and out == 5 and dt >= 0.0, "exactly K steps, the drain inside, a sync on both sides"
    lib.nrf_profile_enable(1)
    try:
        assert lib.nrf_profile_is_enabled() == 1
        with pytest.raises(timing.ProfilingEnabledError):
            timing.timed_region(lib, lambda: None, lambda: None, lambda: None, 1)
    finally:
        lib.nrf_profile_enable(0)
    # a step that switches the bracketing on mid-region is caught as well
    with pytest.raises(timing.ProfilingEnabledError):
        try:
            timing.timed_region(lib, lambda: lib.nrf_profile_enable(1), lambda: None, lambda: None, 1)
        finally:
            lib.nrf_profile_enable(0)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")).read()
    assert "timing.timed_region(lib, step, drain, sync, steps)" in src and not re.search(r"timed_run\([^)]*profile\s*=", src), "the headline goes through timed_region; no profile= switch on it"
    # the lane choice: interleaved blocks through the same refusing region, a tie goes to fewer lanes, the winner is left set
    state = {"lanes": 0}
    cost = {1: 0.004, 2: 0.003}
    import time as _t
    win, by = timing.choose_lanes(lib, lambda n: state.update(lanes=n), lambda: _t.sleep(cost[state["lanes"]]), lambda: None, lambda: None, lambda x: x, frames=3, rounds=2)
    assert win == 2 and state["lanes"] == 2 and by[1] > by[2]
    cost[2] = 0.016
    win, _ = timing.choose_lanes(lib, lambda n: state.update(lanes=n), lambda: _t.sleep(cost[state["lanes"]]), lambda: None, lambda: None, lambda x: x, frames=3, rounds=1)
    assert win == 1 and state["lanes"] == 1, "a second lane that does not pay is not used"


def test_inline_asm_never_reads_a_matrix_packed_or_transcendental_result():
    """tools/asm_input_lint.py over every kernel source: the compiler pads the hazards of its own instructions and does not look into inline asm, so an asm
    instruction that reads what a matrix, packed-fp32 or transcendental instruction wrote is right alone and wrong beside other waves (round 3, DESIGN section 9:
    the baked hash lookup with packed weight multiplies).  Compiles for gfx950 (no GPU needed), about a minute on 8 cores."""
    import shutil, subprocess, sys
    if not os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "asm_input_lint.py")], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "hash_fast" in r.stdout and "mlp_small_mfma" in r.stdout


def test_committed_counter_summary_is_plausible_and_matches_the_kernel_sources():
    """profiles/pmc_latest.json (what bench.py's roofline.traffic is computed from), when it is stamped with the hashes of the CURRENT kernel sources (else the bench
    reports traffic as null): its HBM bytes per point are of the right order -- a re-take in round 4 had counted ~70 settling frames into two frames' worth of points (3 334 B per point for
    the hash encode instead of ~160) and nothing noticed."""
    import json
    import os
    from benchlib import roofline as RF
    d = json.load(open(os.path.join(RF.ROOT, "profiles", "pmc_latest.json")))
    import pytest
    stale = [k for k, h in d["_meta"]["kernel_source_sha256_16"].items() if h != RF.kernel_source_hash(k)]
    if stale:           # allowed mid-round (bench.py then reports traffic as null, with the reason); the summary is re-taken with tools/gpu_pmc_round.sh before a round closes
        pytest.skip(f"kernel sources changed since the counter passes at {d['_meta']['commit']}: {stale}")
    bounds = {"hash_encode (k_hash_cu_lm)": (60.0, 600.0),           # 588 B gathered per point algorithmically, caches serve most of the lines
              "mlp_small (k_mlp_small_mfma)": (40.0, 200.0),         # ~92 B per point algorithmically
              "sigma_small_f32 (k_sigma_small_f32)": (40.0, 400.0)}
    for k, (lo, hi) in bounds.items():
        v = d[k]["hbm_bytes_per_point"]
        assert lo < v < hi, (k, v)
        t, why = RF.pmc_traffic(k, 1e6)
        assert t is not None and abs(t - v * 1e6) < 1e-3 * v * 1e6, (k, t, why)
