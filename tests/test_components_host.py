"""Connected components without a GPU: the four entry points are declared and exported, the numpy restatement (tests/components_ref.py) agrees with scipy on
every shape the GPU tests use, those shapes are what they claim to be, and FilterComponents (with labels given it calls no kernel) on a hand-made mesh."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import components_ref as R
import mesh_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["nrf_mesh_components_workspace_bytes", "nrf_mesh_components", "nrf_lattice_components_workspace_bytes", "nrf_lattice_components"]


def test_entry_points_declared_and_exported():
    from nerfpp_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nerfpp_hip.h")).read()
    declared = re.findall(r"NRF_API\s+[\w\s\*]+?\b(nrf_\w+)\s*\(", hdr)
    at = declared.index("nrf_isosurface_emit")
    assert declared[at + 1:at + 5] == NAMES, "the section follows the isosurface block"
    at = _lib.SYMBOLS.index("nrf_isosurface_emit")
    assert _lib.SYMBOLS[at + 1:at + 5] == NAMES
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), f"libnerfpp_hip.so does not export {name}"
    # the size functions are host code: one layout, measured
    lib.nrf_mesh_components_workspace_bytes.restype = lib.nrf_lattice_components_workspace_bytes.restype = C.c_size_t
    small = lib.nrf_mesh_components_workspace_bytes(C.c_int64(1000), C.c_int64(5))
    assert small >= 256 + 4 * 1000 + 4 * 4 and small % 256 == 0
    assert lib.nrf_lattice_components_workspace_bytes(10, 10, 10) == small
    assert lib.nrf_mesh_components_workspace_bytes(C.c_int64(-1), C.c_int64(0)) == 0 and lib.nrf_lattice_components_workspace_bytes(0, 4, 4) == 0
    assert lib.nrf_lattice_components_workspace_bytes(2048, 2048, 512) == 0          # 2^31 points


def _scipy_labels(n, a, b, takes_part):
    """scipy's components of the same graph, renumbered by smallest member."""
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    g = sp.coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n, n))
    _, lab = connected_components(g, directed=False)
    first = np.full(lab.max(initial=-1) + 1, n, np.int64)
    np.minimum.at(first, lab, np.arange(n))               # smallest member of each scipy component
    return R.canonical(first[lab], takes_part)


@pytest.mark.parametrize("name", ["strip", "tetrahedra", "joined_last", "two_strips", "degenerate"])
def test_reference_equals_scipy_on_the_mesh_shapes(name):
    faces, v, k = R.mesh_cases()[name]
    f = faces.astype(np.int64)
    assert f.min() >= 0 and f.max() < v
    used = np.zeros(v, bool)
    used[f.reshape(-1)] = True
    labels, kk = R.mesh_components(faces, v)
    assert kk == k and labels.max() == k - 1 and ((labels == -1) == ~used).all()
    assert (labels[f[:, 0]] == labels[f[:, 1]]).all() and (labels[f[:, 1]] == labels[f[:, 2]]).all()
    ref, kr = _scipy_labels(v, np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]]), used)
    assert kr == k and (ref == labels).all()
    if name == "tetrahedra":
        assert (~used).sum() == 37
    if name == "joined_last":
        assert R.mesh_components(faces[:-1], v)[1] == 2, "only the last face joins the two strips"
    if name == "degenerate":
        assert (f[:, 0] == f[:, 1]).sum() > 1000 and ((f[:, 0] == f[:, 1]) & (f[:, 1] == f[:, 2])).sum() > 1000
        assert len(np.unique(f, axis=0)) < len(f) - 1000


@pytest.mark.parametrize("connectivity", [6, 14, 26])
def test_reference_equals_scipy_on_the_lattice_shapes(connectivity):
    assert len(R.offsets(connectivity)) == connectivity // 2
    both = R.offsets(connectivity) + [tuple(-v for v in o) for o in R.offsets(connectivity)]
    assert len(set(both)) == connectivity and all(max(map(abs, o)) == 1 for o in both)
    for name, m in R.lattice_masks().items():
        labels, k = R.lattice_components(m, connectivity)
        a, b = R.lattice_edges(m, connectivity)
        ref, kr = _scipy_labels(m.size, a, b, m.reshape(-1))
        assert kr == k and (ref.reshape(m.shape) == labels).all(), name
        assert ((labels == -1) == ~m).all()


def test_the_lattice_shapes_are_what_they_claim():
    for c in (6, 14, 26):
        m = R.percolation_mask(c)
        assert m.shape == (29, 33, 40)
        labels, k = R.lattice_components(m, c)
        largest = np.bincount(labels[labels >= 0]).max()
        print(f"connectivity {c}: p {R.PERCOLATION[c]}, K {k}, largest {largest}, set {m.sum()}")
        assert k >= 50 and 0.2 <= largest / m.sum() <= 0.8, "near percolation: many clusters, one tortuous large one"
    m = R.serpentine(32)
    assert m.shape == (32, 32, 32) and m.sum() > 8000
    for c in (6, 14, 26):
        assert R.lattice_components(m, c)[1] == 1
    a, b = R.lattice_edges(m, 6)
    degree = np.bincount(np.concatenate([a, b]), minlength=m.size)[m.reshape(-1)]
    assert (degree == 1).sum() == 2 and (degree <= 2).all(), "a path under 6: two ends, no branch"
    w = R.wrap_mask(40, 33, 29)
    flat = np.nonzero(w.reshape(-1))[0]
    assert (np.diff(flat) == 1).sum() == len(flat) // 2 > 200, "every point has its partner next to it in memory"
    for c in (6, 14, 26):
        assert R.lattice_components(w, c)[1] == w.sum(), "and no neighbour on the lattice"


def test_known_mesh_answer_in_the_restatements():
    f, box = R.known_field()
    v, fc, _, _ = M.isosurface(f, box, 0.0)
    assert (len(v), len(fc)) == (3238, 6468)
    labels, k = R.mesh_components(fc, len(v))
    assert k == 3 and np.bincount(labels[fc[:, 0]]).tolist() == [1536, 600, 4332]
    assert R.lattice_components(f > 0, 14)[1] == 3


# ------------------------------------------------------------------------------------ FilterComponents on the host
def _hand_mesh():
    """Three components over 12 vertices, vertex 4 unused, ids interleaved: A = {0, 2, 5, 7} (3 faces), B = {1, 3, 6} (1 face), C = {8, 9, 10, 11} (3 faces)."""
    from nerfpp_amd.mesh import Mesh
    faces = torch.tensor([[8, 9, 10], [0, 2, 5], [1, 3, 6], [2, 5, 7], [9, 10, 11], [7, 0, 2], [11, 8, 9]], dtype=torch.int32)
    v = torch.arange(36, dtype=torch.float32).reshape(12, 3)
    return Mesh(v, faces, -v, v / 36.0, torch.stack([torch.arange(12.0), 12 - torch.arange(12.0)], 1))


def _check_sub(full, sub, old, faces_kept):
    old = torch.tensor(old)
    assert torch.equal(sub.Vertices, full.Vertices[old]) and torch.equal(sub.Normals, full.Normals[old])
    assert torch.equal(sub.Colors, full.Colors[old]) and torch.equal(sub.Relevancy, full.Relevancy[old])
    assert sub.Faces.dtype == torch.int32
    assert torch.equal(old[sub.Faces.to(torch.int64)], full.Faces[torch.tensor(faces_kept)].to(torch.int64)), "faces in their original order, re-indexed"


def test_filter_components_on_a_hand_made_mesh():
    from nerfpp_amd.mesh import FilterComponents, Mesh
    m = _hand_mesh()
    labels, k = R.mesh_components(m.Faces.numpy(), 12)
    assert k == 3 and labels.tolist() == [0, 1, 0, 1, -1, 0, 1, 0, 2, 2, 2, 2]
    lab = torch.from_numpy(labels)
    a, b, c = [0, 2, 5, 7], [1, 3, 6], [8, 9, 10, 11]
    # sizes are face counts (3, 1, 3); the tie between A and C goes to the lower label
    _check_sub(m, FilterComponents(m, keep_largest=1, labels=lab), a, [1, 3, 5])
    _check_sub(m, FilterComponents(m, keep_largest=2, labels=lab), a + c, [0, 1, 3, 4, 5, 6])
    _check_sub(m, FilterComponents(m, keep_largest=3, labels=lab), sorted(a + b + c), list(range(7)))
    _check_sub(m, FilterComponents(m, keep_largest=7, labels=lab), sorted(a + b + c), list(range(7)))
    _check_sub(m, FilterComponents(m, min_faces=2, labels=lab), a + c, [0, 1, 3, 4, 5, 6])
    _check_sub(m, FilterComponents(m, labels=lab), sorted(a + b + c), list(range(7)))            # no criterion: only the unused vertex goes
    # the criteria intersect: B is among the 3 largest but too small, C is large enough but not the largest
    _check_sub(m, FilterComponents(m, keep_largest=3, min_faces=2, labels=lab), a + c, [0, 1, 3, 4, 5, 6])
    _check_sub(m, FilterComponents(m, keep_largest=1, min_faces=3, labels=lab), a, [1, 3, 5])
    for empty in (FilterComponents(m, keep_largest=0, labels=lab), FilterComponents(m, min_faces=4, labels=lab)):
        assert empty.Vertices.shape == (0, 3) and empty.Faces.shape == (0, 3) and empty.Colors.shape == (0, 3) and empty.Relevancy.shape == (0, 2)
    # attributes that are absent stay absent; labels may come as numpy
    bare = FilterComponents(Mesh(m.Vertices, m.Faces, m.Normals), keep_largest=1, labels=labels)
    assert bare.Colors is None and bare.Relevancy is None and torch.equal(bare.Vertices, m.Vertices[torch.tensor(a)])


def test_segment_mesh_shares_the_sub_mesh_helper_unchanged():
    """SegmentMesh returns what it returned before the helper moved: checked on the hand-made mesh against the rule written out."""
    from nerfpp_amd.query import SegmentMesh
    m = _hand_mesh()
    rel = m.Relevancy.flip(1).contiguous()               # column 0 = 12 - i: vertices 0 .. 7 pass 4.5
    s = SegmentMesh(m, rel, 4.5)
    old = torch.tensor([0, 1, 2, 3, 5, 6, 7])
    assert torch.equal(s.Vertices, m.Vertices[old]) and torch.equal(s.Normals, m.Normals[old]) and torch.equal(s.Colors, m.Colors[old])
    assert torch.equal(s.Relevancy, rel[old])
    assert torch.equal(old[s.Faces.to(torch.int64)], m.Faces[torch.tensor([1, 2, 3, 5])].to(torch.int64))
