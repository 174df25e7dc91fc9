"""LeRF relevancy in 3D without a GPU: the float64 restatement (tests/lerf_query_ref.py) in both forms against each other and against the C oracle, SegmentMesh on
CPU tensors, and the PLY relevancy property."""
import os

import numpy as np
import pytest
import torch

import lerf_query_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(manifest):
    from nerfpp_amd import synth
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "lerf.npz")))
    return synth.blob_from_manifest(manifest["lerf"]), g["x"]


@pytest.mark.parametrize("n_neg", [0, 1, 4, 31])
@pytest.mark.parametrize("positive_id", [0, 2])
def test_restatement_forms_agree_and_match_the_oracle(golden, n_neg, positive_id):
    from oracle import capi as O
    blob, x = golden
    pos, neg = Q.unit_prompts(3, 17 + n_neg), Q.unit_prompts(n_neg, 91 + n_neg)
    direct = Q.relevancy_direct(blob, x, pos, neg, positive_id).numpy()
    proj = Q.relevancy_projection(blob, x, pos, neg, positive_id).numpy()
    assert np.abs(direct - proj).max() <= 1e-12
    ref = O.relevancy(O.lerf(blob, x)[:, :768], pos, neg.reshape(-1, 768), positive_id)
    assert np.abs(direct - ref).max() <= 1e-6
    if n_neg == 0:
        assert not direct.any()
    else:
        assert np.allclose(direct.sum(1), 1.0)


def test_restatement_sigma_is_the_oracle_sigma_net(golden):
    from oracle import capi as O
    blob, x = golden
    sig = Q.head(blob, x)[0].numpy()
    assert np.abs(sig - O.lerf_sigma_net(blob, x)[:, 0]).max() <= 1e-5 * max(1.0, np.abs(sig).max())


def _square_mesh():
    from nerfpp_amd.mesh import Mesh
    # 3 x 2 vertex strip, four triangles; vertex 4 is low
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [1, 1, 0], [2, 1, 0]], dtype=torch.float32)
    f = torch.tensor([[0, 1, 3], [1, 4, 3], [1, 2, 4], [2, 5, 4]], dtype=torch.int32)
    n = torch.tensor([[0, 0, 1]] * 6, dtype=torch.float32)
    c = torch.linspace(0, 1, 18).reshape(6, 3)
    return Mesh(v, f, n, c)


def test_segment_mesh_keeps_faces_whose_vertices_all_pass_and_compacts_in_order():
    from nerfpp_amd.query import SegmentMesh
    m = _square_mesh()
    rel = torch.tensor([[0.9, 0.1], [0.8, 0.2], [0.7, 0.3], [0.6, 0.4], [0.1, 0.9], [0.95, 0.05]])
    s = SegmentMesh(m, rel, 0.5)
    assert s.Faces.dtype == torch.int32 and s.Vertices.device.type == "cpu"
    # only face 0 (vertices 0, 1, 3) has every vertex >= 0.5
    assert s.Faces.tolist() == [[0, 1, 2]]
    assert s.Vertices.tolist() == m.Vertices[[0, 1, 3]].tolist()
    assert torch.equal(s.Colors, m.Colors[[0, 1, 3]]) and torch.equal(s.Normals, m.Normals[[0, 1, 3]])
    assert torch.equal(s.Relevancy, rel[[0, 1, 3]])
    # threshold 0: everything; above every value: nothing
    s_all = SegmentMesh(m, rel, 0.0)
    assert s_all.Faces.tolist() == m.Faces.tolist() and torch.equal(s_all.Vertices, m.Vertices)
    s_none = SegmentMesh(m, rel, 2.0)
    assert s_none.Faces.shape == (0, 3) and s_none.Vertices.shape == (0, 3)


def test_segment_mesh_drops_vertices_of_no_kept_face():
    from nerfpp_amd.query import SegmentMesh
    m = _square_mesh()
    rel = torch.tensor([[0.9, 0.1], [0.9, 0.1], [0.9, 0.1], [0.1, 0.9], [0.9, 0.1], [0.9, 0.1]])
    s = SegmentMesh(m, rel, 0.5)
    # faces 2 (1, 2, 4) and 3 (2, 5, 4) pass; vertex 0 passes but no kept face uses it
    assert s.Vertices.tolist() == m.Vertices[[1, 2, 4, 5]].tolist()
    assert s.Faces.tolist() == [[0, 1, 2], [1, 3, 2]]


def _read_ply(path):
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    return data[:end].decode("ascii").splitlines(), data[end:]


def test_save_ply_relevancy_property_round_trips(tmp_path):
    from nerfpp_amd.mesh import SavePLY
    m = _square_mesh()
    m.Relevancy = torch.tensor([[0.9, 0.1], [0.8, 0.2], [0.7, 0.3], [0.6, 0.4], [0.1, 0.9], [0.95, 0.05]])
    p = tmp_path / "r.ply"
    SavePLY(str(p), m)
    head, body = _read_ply(p)
    props = [h for h in head if h.startswith("property")]
    assert props[:10] == ["property float x", "property float y", "property float z", "property float nx", "property float ny", "property float nz",
                          "property uchar red", "property uchar green", "property uchar blue", "property float relevancy"]
    dt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                   ("relevancy", "<f4")])
    rec = np.frombuffer(body[:6 * dt.itemsize], dtype=dt)
    assert np.array_equal(rec["relevancy"], m.Relevancy[:, 0].numpy())
    assert np.array_equal(rec["x"], m.Vertices[:, 0].numpy())
    fr = np.frombuffer(body[6 * dt.itemsize:], dtype=np.dtype([("n", "u1"), ("idx", "<i4", (3,))]))
    assert fr["idx"].tolist() == m.Faces.tolist()


def test_save_ply_without_relevancy_is_unchanged(tmp_path):
    from nerfpp_amd.mesh import SavePLY
    m = _square_mesh()
    a, b = tmp_path / "a.ply", tmp_path / "b.ply"
    SavePLY(str(a), m)
    m2 = _square_mesh()
    m2.Relevancy = None
    SavePLY(str(b), m2)
    assert a.read_bytes() == b.read_bytes()
    assert b"relevancy" not in a.read_bytes()
