"""Property tests of the numpy restatement of exa_hip_isosurface's contract (tests/isomesh_ref.py) on analytic lattices:
the restatement is the checker of the GPU tests, so it is checked here on its own, without a GPU."""
import numpy as np

import isomesh_ref as ref

F = np.float32


def _lattice(dims, lo, hi):
    ax = ref.lattice_axes(lo, hi, dims)
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return x, y, z


def test_tet_rules_cover_every_case_once():
    # every pattern with both signs gives 1 or 2 triangles over crossing edges only, each edge of a triangle distinct
    for perm in ref.PERMS:
        assert sorted(ref.tet_corners(perm)) == sorted(set(ref.tet_corners(perm))) and ref.tet_corners(perm)[3] == 7
        for pat in range(16):
            tris = ref.tet_triangles(pat, perm)
            ninside = bin(pat).count("1")
            assert len(tris) == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[ninside]
            for t in tris:
                assert len(set(frozenset(e) for e in t)) == 3
                for x, y in t:
                    assert ((pat >> x) & 1) != ((pat >> y) & 1)


def test_radial_field_is_a_closed_oriented_sphere():
    n = 14
    lo, hi = (0.0, 0.0, 0.0), (float(n), float(n), float(n))
    x, y, z = _lattice((n, n, n), lo, hi)
    c = n / 2.0
    r = np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2)
    V = (F(1.0) - r / F(5.0)).astype(F)             # 1 - r/R: the surface V == 0 is the sphere of radius 5 cells
    verts, tris = ref.extract(V, lo, hi, 0.0)
    assert len(tris) > 2000 and len(tris) == 2 * len(verts) - 4      # a closed surface of genus 0: E = 3F/2, V - E + F = 2
    assert not ref.degenerate(verts, tris).any()
    rep = ref.closed_manifold_report(len(verts), tris)
    assert rep == dict(boundary=0, repeated=0, euler=2), rep
    assert ref.unreferenced_vertices(len(verts), tris) == 0
    assert len(np.unique(verts, axis=0)) == len(verts)
    # the lower values are outside: every normal points away from the centre (float64)
    nrm = ref.normals64(verts, tris)
    centroid = verts.astype(np.float64)[tris].mean(axis=1)
    assert np.all(np.einsum("ij,ij->i", nrm, centroid - c) > 0)
    # and the vertices sit on the sphere to within the linear interpolation's error on a unit lattice
    rad = np.linalg.norm(verts.astype(np.float64) - c, axis=1)
    assert np.all(np.abs(rad - 5.0) < 0.15), (rad.min(), rad.max())


def test_orientation_equals_the_geometric_one_in_every_tet_case():
    # one cube, a linear field through it in general position for every sign pattern a tet can take: the normal of every
    # triangle points down the gradient
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(400):
        g = rng.normal(size=3)
        off = rng.uniform(-1.5, 1.5)
        ax = np.arange(2, dtype=np.float64) + 0.5
        z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
        V = (g[0] * x + g[1] * y + g[2] * z - (g.sum() + off)).astype(F)
        inside = V >= 0
        verts, tris = ref.extract(V, (0, 0, 0), (2, 2, 2), 0.0)
        if len(tris) == 0:
            continue
        for ti, perm in enumerate(ref.PERMS):
            cc = ref.tet_corners(perm)
            pat = sum(int(inside.reshape(-1)[cc[v]]) << v for v in range(4))
            seen.add((ti, pat))
        nrm = ref.normals64(verts, tris)
        assert np.all(nrm @ g < 0), (g, off)
    assert len(seen) >= 6 * 14          # all 6 x 14 mixed cases met (plus the uniform ones)


def test_linear_field_puts_every_vertex_on_the_plane():
    dims = (11, 9, 7)
    lo, hi = (-1.0, 0.5, 2.0), (4.5, 5.0, 9.0)
    x, _, _ = _lattice(dims, lo, hi)
    V = x.astype(F)
    iso = F(1.7)
    verts, tris = ref.extract(V, lo, hi, iso)
    assert len(tris) > 0
    # x == iso to within 1 ulp of the lattice coordinate
    ulp = np.spacing(np.abs(ref.lattice_axes(lo, hi, dims)[0]).max().astype(F))
    assert np.all(np.abs(verts[:, 0].astype(np.float64) - float(iso)) <= float(ulp)), np.abs(verts[:, 0] - iso).max()
    rep = ref.closed_manifold_report(len(verts), tris)
    assert rep["repeated"] == 0 and ref.unreferenced_vertices(len(verts), tris) == 0
    nrm = ref.normals64(verts, tris)
    assert np.all(nrm[:, 0] < 0)                    # toward the lower values


def test_lattice_value_equal_to_iso_keeps_zero_area_triangles():
    n = 8
    x, y, z = _lattice((n, n, n), (0, 0, 0), (n, n, n))
    V = (x + F(0.25) * y - F(0.5) * z).astype(F)
    iso = V[3, 4, 2]
    verts, tris = ref.extract(V, (0, 0, 0), (n, n, n), iso)
    assert ref.degenerate(verts, tris).any()
    assert ref.repeated_directed_edges(tris[~ref.degenerate(verts, tris)]) == 0
    assert ref.unreferenced_vertices(len(verts), tris) == 0


def test_nan_cubes_emit_nothing_and_leave_no_loose_vertices():
    n = 16
    rng = np.random.default_rng(11)
    x, y, z = _lattice((n, n, n), (0, 0, 0), (n, n, n))
    c = n / 2.0
    V = (F(1.0) - np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) / F(5.5)).astype(F)
    holes = rng.random(V.shape) < 0.03
    V[holes] = np.nan
    V[:, :, :2] = np.inf
    verts, tris = ref.extract(V, (0, 0, 0), (n, n, n), 0.0)
    assert len(tris) > 200
    assert not ref.valid_cubes(V).all() and ref.valid_cubes(V).any()
    assert np.isfinite(verts).all()
    assert ref.repeated_directed_edges(tris) == 0
    assert ref.unreferenced_vertices(len(verts), tris) == 0
    # no triangle comes from an invalid cube: every triangle's vertices lie within one valid cube
    valid = ref.valid_cubes(V)
    cell = np.floor(verts[tris].astype(np.float64).min(axis=1) - 0.5 + 1e-6).astype(int)
    cell = np.clip(cell, 0, n - 2)
    assert valid[cell[:, 2], cell[:, 1], cell[:, 0]].all()


def test_two_runs_give_the_same_bytes():
    rng = np.random.default_rng(3)
    V = rng.normal(size=(9, 10, 11)).astype(F)
    a = ref.extract(V, (0, 0, 0), (1, 2, 3), 0.1)
    b = ref.extract(V.copy(), (0, 0, 0), (1, 2, 3), 0.1)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert ref.repeated_directed_edges(a[1]) == 0 and ref.unreferenced_vertices(len(a[0]), a[1]) == 0
