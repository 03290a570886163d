"""The NumPy restatement of TSDF fusion and the marching-tetrahedra mesh (tests/tsdf_ref.py) on its own, no GPU: the mesh's
topology, orientation, accuracy and validity rule as include/lcgs_hip.h states them, and the cap on the integrate cases' undecided
(sample, view) pairs -- the draws tests/test_gpu_tsdf.py holds the kernels to."""
import numpy as np
import pytest

import tsdf_ref as R

_MESHES = {}


def _mesh(name, dt=np.float32):
    if (name, dt) not in _MESHES:
        t, w, rgb, origin, voxel, dims = R.mesh_case(name)
        _MESHES[name, dt] = R.mesh(t, w, origin, voxel, dims, rgb=rgb, dt=dt)
    return _MESHES[name, dt]


@pytest.mark.parametrize("name, euler", [("sphere", 2), ("torus", 0), ("zeros", 2)])
def test_closed_manifold_with_the_right_euler_characteristic(name, euler):
    """every edge in exactly two triangles, V - E + F as the surface's genus says -- samples that are exactly 0 included"""
    m = _mesh(name)
    V, F = len(m["vertices"]), len(m["triangles"])
    edges, counts = R.edges_of(m["triangles"])
    assert F > 1000 and (counts == 2).all(), np.unique(counts)
    assert V - len(edges) + F == euler
    assert len(np.unique(m["triangles"])) == V  # every vertex is used
    assert (m["triangles"][:, 0] < m["triangles"][:, 1]).all() and (m["triangles"][:, 0] < m["triangles"][:, 2]).all()
    assert (np.diff(m["keys"][:, 0] * 8 + m["keys"][:, 1]) > 0).all()  # numbered in ascending key order, once each


@pytest.mark.parametrize("name", ["sphere", "torus", "zeros", "clipped"])
def test_vertices_lie_on_the_seven_edge_directions(name):
    t, w, rgb, origin, voxel, dims = R.mesh_case(name)
    m = _mesh(name, np.float64)
    X = R.lattice(origin, voxel, dims, np.float64)
    s_lo, d = m["keys"][:, 0], m["keys"][:, 1]
    assert ((d >= 1) & (d <= 7)).all()
    step = np.stack([d & 1, (d >> 1) & 1, (d >> 2) & 1], axis=1).astype(np.float64)
    rel = (m["vertices"] - X[s_lo]) / float(np.float32(voxel))
    lam = (rel * step).sum(axis=1) / step.sum(axis=1)
    assert (lam >= 0).all() and (lam <= 1).all()
    assert np.abs(rel - lam[:, None] * step).max() <= 1e-9


@pytest.mark.parametrize("name", ["sphere", "torus", "zeros", "clipped", "hole"])
def test_orientation_points_from_inside_to_outside(name):
    """binary64: every triangle of area > 1e-12 has a normal with a positive dot product with (mean outside corner - mean inside
    corner) of its tetrahedron; the closed ones enclose a positive volume"""
    m = _mesh(name, np.float64)
    v = m["vertices"][m["triangles"]]
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    big = np.linalg.norm(nrm, axis=1) * 0.5 > 1e-12
    assert big.sum() > 0.9 * len(nrm) or name == "zeros"
    assert (np.einsum("ij,ij->i", nrm, m["tri_dir"])[big] > 0).all()
    if name in ("sphere", "torus", "zeros"):
        assert R.signed_volume(m["vertices"], m["triangles"]) > 0


def test_enclosed_volume_of_the_sphere():
    """the binary64 mesh of the radius-6.37-voxel sphere on 20^3 encloses 4/3 pi r^3 less 1.2335 % (measured; an inscribed
    piecewise-linear surface): asserted at 1.5 x that"""
    t, w, rgb, origin, voxel, dims = R.mesh_case("sphere")
    m = _mesh("sphere", np.float64)
    exact = 4.0 / 3.0 * np.pi * (6.37 * float(np.float32(voxel))) ** 3
    dev = abs(R.signed_volume(m["vertices"], m["triangles"]) - exact) / exact
    print(f"relative deviation of the enclosed volume: {dev:.6f}")
    assert dev <= 1.5 * 0.012335


def test_zero_weight_block_opens_the_mesh_exactly_there():
    t, w, rgb, origin, voxel, dims = R.mesh_case("hole")
    nx, ny, nz = dims
    hole, full = _mesh("hole"), _mesh("sphere")
    good = (w >= 1.0).reshape(nz, ny, nx)
    valid = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for c in range(8):
        valid &= good[R._corner_slices(dims, c)]
    assert not valid.all()
    # no vertex on an edge that touches no valid cell
    for s_lo, d in hole["keys"]:
        lo = np.array([s_lo % nx, (s_lo // nx) % ny, s_lo // (nx * ny)])
        step = np.array([d & 1, (d >> 1) & 1, (d >> 2) & 1])
        cells = [(i, j, k) for i in range(lo[0] - 1 + step[0], lo[0] + 1) for j in range(lo[1] - 1 + step[1], lo[1] + 1)
                 for k in range(lo[2] - 1 + step[2], lo[2] + 1) if 0 <= i < nx - 1 and 0 <= j < ny - 1 and 0 <= k < nz - 1]
        assert any(valid[k, j, i] for i, j, k in cells), (s_lo, d)
    # the triangles are the full sphere's triangles of the cells that stayed valid, the same bits in the same order
    cell_ok = np.zeros(nx * ny * nz, bool)
    kk, jj, ii = np.nonzero(valid)
    cell_ok[(kk * ny + jj) * nx + ii] = True
    keep = cell_ok[full["tri_cell"]]
    assert 0 < keep.sum() < len(keep) and keep.sum() == len(hole["triangles"])
    assert np.array_equal(full["vertices"][full["triangles"][keep]].view(np.uint32), hole["vertices"][hole["triangles"]].view(np.uint32))
    # open exactly along the block: every boundary edge belongs to a triangle whose cell has a dropped neighbour
    edges, counts = R.edges_of(hole["triangles"])
    assert set(np.unique(counts)) == {1, 2}
    boundary = {tuple(e) for e in edges[counts == 1]}
    tri = hole["triangles"]
    for f in range(len(tri)):
        a, b, c = tri[f]
        if any(tuple(sorted(e)) in boundary for e in ((a, b), (b, c), (c, a))):
            s = hole["tri_cell"][f]
            i, j, k = s % nx, (s // nx) % ny, s // (nx * ny)
            near = valid[max(k - 1, 0):k + 2, max(j - 1, 0):j + 2, max(i - 1, 0):i + 2]
            assert not near.all(), (f, i, j, k)


def test_single_cells_and_degenerate_lattices():
    for name, (nv, nt) in {"cell_one": (7, 6), "cell_inside": (0, 0), "flat": (0, 0)}.items():
        m = _mesh(name)
        assert (len(m["vertices"]), len(m["triangles"])) == (nv, nt), name
    m = _mesh("cell_mixed")  # -0.0f is not inside
    assert len(m["triangles"]) > 0 and np.isfinite(m["vertices"]).all()


@pytest.mark.parametrize("lattice", list(R.LATTICES))
def test_undecided_pairs_of_the_integrate_cases_are_capped(lcgs, lattice):
    """a condition on the draws: at most 0.5 % of the (sample, view) pairs of the GPU tests' integrate cases sit within 16 ulp of a
    pixel edge or a threshold (generic look-at poses: no optical axis through a lattice line)"""
    origin, voxel, dims = R.LATTICES[lattice]
    count = 2 * R.VIEW_CHUNK + 3 if lattice == "odd" else 5
    ref = R.integrate(lcgs, origin, voxel, dims, R.views(lcgs, count), R.CFG)
    for first in range(0, count, 5):
        und = ref["undecided"][:, first:first + 5]
        assert und.mean() <= 0.005, (first, und.sum(), und.size)
    if lattice != "one":
        assert ref["applied"][:, :5].any(axis=0).sum() >= 4 and (ref["weight"] >= 2).any()
    else:
        assert ref["applied"].any()
