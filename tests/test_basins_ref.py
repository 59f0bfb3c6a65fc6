"""The numpy restatement of exa_hip_basins' contract (tests/basins_ref.py) checked on its own, without a GPU: against the
regions' restatement where minDepth = inf makes the basins the regions, against scipy's maximum filter where minDepth = 0
makes the basins the local maxima, on hand cases on a line of points, and through the identities of the table."""
import numpy as np
import pytest

import basins_ref as ref
import regions_ref
from test_regions_ref import _field

INF = float("inf")


@pytest.mark.parametrize("below", [False, True])
@pytest.mark.parametrize("faces", [False, True])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_with_infinite_depth_the_basins_are_the_regions(seed, faces, below):
    V = _field(seed)
    iso = (0.8 if seed != 3 else 1.0) * (-1 if below else 1)       # as there: a fifth of the points inside
    want, T, s = regions_ref.regions(V, iso, below=below, faces=faces)
    labels, B, sb, raw, rounds = ref.basins(V, iso, INF, below=below, faces=faces)
    assert len(T) > 3 and raw > len(T) and 1 <= rounds <= 64
    assert ref.same_partition(labels, want) and len(B) == len(T) and sb == s
    # the same sets, numbered by the peak instead of the first point
    order = np.argsort(B["first"])
    for name in regions_ref.REGION.names:
        assert np.array_equal(B[name][order], T[name]), name
    assert np.all(B["neighbour"] == -1) and np.all(np.isnan(B["saddle"])) and np.all(np.isposinf(B["depth"]))


@pytest.mark.parametrize("below", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_with_no_depth_the_peaks_are_the_local_maxima(seed, below):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(seed)
    V = rng.permutation(13 * 17 * 19).astype(np.float32).reshape(13, 17, 19) - 2000.0      # distinct values
    foot = ndimage.generate_binary_structure(3, 1)
    iso = -1e9 if not below else 1e9                               # every point inside
    W = -V if below else V
    peaks = ndimage.maximum_filter(W, footprint=foot, mode="constant", cval=-np.inf) == W
    labels, B, _, raw, rounds = ref.basins(V, iso, 0.0, below=below, faces=True)
    assert rounds == 0 and raw == len(B) == peaks.sum() > 10
    assert np.array_equal(B["argMin" if below else "argMax"], np.nonzero(peaks.reshape(-1))[0])
    assert np.array_equal(np.nonzero(ref.up_links(V, iso, below, True) == np.arange(V.size))[0], np.nonzero(peaks.reshape(-1))[0])


def _line(values):
    return np.asarray(values, np.float32).reshape(1, 1, -1)


def test_two_peaks_and_a_pass():
    V = _line([1, 3, 2, 5, 1])
    labels, B, _, raw, rounds = ref.basins(V, 0.0, 0.5)
    assert (raw, len(B), rounds) == (2, 2, 0)
    assert labels.reshape(-1).tolist() == [0, 0, 1, 1, 1]         # the pass climbs to the greater neighbour
    assert B["neighbour"].tolist() == [1, 0] and B["saddle"].tolist() == [2.0, 2.0] and B["depth"].tolist() == [1.0, 3.0]
    assert B["argMax"].tolist() == [1, 3] and B["first"].tolist() == [0, 2]
    labels, B, _, raw, rounds = ref.basins(V, 0.0, 1.5)
    assert (raw, len(B), rounds) == (2, 1, 1) and np.all(labels == 0)
    assert B["neighbour"][0] == -1 and np.isnan(B["saddle"][0]) and np.isposinf(B["depth"][0]) and B["argMax"][0] == 3
    # depth < minDepth is strict
    assert len(ref.basins(V, 0.0, 1.0)[1]) == 2
    # minima: the mirror image
    labels, B, _, raw, rounds = ref.basins(-V, 0.0, 1.5, below=True)
    assert (raw, len(B), rounds) == (2, 1, 1) and B["argMin"][0] == 3


def test_equal_peaks_the_smaller_index_survives():
    V = _line([4, 1, 4])
    labels, B, _, raw, rounds = ref.basins(V, 0.0, 0.0)
    assert raw == 2 and labels.reshape(-1).tolist() == [0, 0, 1]   # the pass ties too: to the smaller index
    labels, B, _, raw, rounds = ref.basins(V, 0.0, 10.0)
    assert (raw, len(B), rounds) == (2, 1, 1) and B["argMax"][0] == 0 and B["max"][0] == 4.0


def test_a_plateau_is_several_raw_basins_and_one_after_any_depth():
    V = _line([2, 2, 2, 2, 2, 2, 2])
    labels, B, _, raw, rounds = ref.basins(V, 0.0, 0.0)
    # every point goes to its left neighbour, the chain ends at 0: one raw basin on a line; on a lattice the ties split
    assert raw == 1
    V = np.full((4, 4, 4), 2.0, np.float32)
    V[:, :, 2] = np.nan                                             # two slabs
    V[0, 0, 2] = 1.0                                                # joined by a lower point
    labels, B, _, raw, rounds = ref.basins(V, 0.0, 0.0, faces=True)
    assert raw == len(B) == 2 and np.all(B["depth"] == 1.0)
    W = np.full((3, 3, 3), 2.0, np.float32)
    W[0, 0, 0] = np.nan                                             # the plateau without its first corner: ties split it
    labels, B, _, raw, rounds = ref.basins(W, 0.0, 0.0, faces=True)
    assert raw > 1 and np.all(B["depth"] == 0.0)
    labels, B, _, raw2, rounds = ref.basins(W, 0.0, 1e-30, faces=True)
    assert raw2 == raw and len(B) == 1 and rounds >= 1


def test_a_chain_of_links_is_one_round():
    # 3 links to 5 over the pass 2.5 and 5 to 6 over 4.5, both of depth 0.5, in the same round: the chain is followed
    V = _line([3.0, 2.5, 5.0, 4.5, 6.0])
    labels, B, _, raw, rounds = ref.basins(V, 0.0, 0.75)
    assert (raw, len(B), rounds) == (3, 1, 1) and B["argMax"][0] == 4
    labels, B, _, raw, rounds = ref.basins(_line([3.0, 2.5, 5.0, 4.5, 6.0, 1.0, 9.0]), 0.0, 0.75)
    assert (raw, len(B), rounds) == (4, 2, 1) and B["argMax"].tolist() == [4, 6]


def test_three_peaks_where_the_second_round_is_needed():
    # peaks 2.0, 2.2 and 9.0 with minDepth 1.5.  Round 1: 2.0 joins 2.2 over the pass 1.9 (depth 0.1); the highest pass of 2.2
    # is that same one (depth 0.3) and leads to a lower peak: no link.  Round 2: the union, peak 2.2, now meets 9.0 over the
    # pass 1.0 with depth 1.2: joined.
    V = _line([2.0, 1.9, 2.2, 1.0, 9.0])
    labels, B, _, raw, rounds = ref.basins(V, 0.0, 1.5)
    assert (raw, len(B), rounds) == (3, 1, 2)
    labels, B, _, raw, rounds = ref.basins(V, 0.0, 1.1)
    assert (raw, len(B), rounds) == (3, 2, 1) and B["depth"].tolist() == [np.float32(2.2) - np.float32(1.0), 8.0]


@pytest.mark.parametrize("faces,below,depth", [(False, False, 0.0), (False, False, 20.0), (True, True, 20.0), (True, False, INF)])
def test_identities_of_the_table(faces, below, depth):
    V = _field(7, shape=(11, 12, 13)) * np.float32(37.5)
    V[0, 0, 0], V[0, 0, 1] = 0.0, -0.0
    iso = 0.0
    labels, T, s, raw, rounds = ref.basins(V, iso, depth, below=below, faces=faces)
    mask = regions_ref.inside(V, iso, below)
    assert T["points"].sum() == mask.sum() == (labels >= 0).sum() and np.array_equal(labels >= 0, mask)
    assert 0 < len(T) <= raw and (depth == 0.0) == (rounds == 0) and (len(T) < raw) == (rounds > 0)
    peak = T["argMin" if below else "argMax"]
    assert np.all(np.diff(peak.astype(np.int64)) > 0)             # numbered by the peak
    assert np.all(T["neighbour"] != np.arange(len(T))) and np.all(T["neighbour"] < len(T))
    has = T["neighbour"] >= 0
    assert np.all(T["depth"][has] >= np.float32(depth)) and np.all(np.isposinf(T["depth"][~has])) and np.all(np.isnan(T["saddle"][~has]))
    if depth not in (0.0, INF):
        assert has.any() and 1 < len(T) < raw
    flat, lab = V.reshape(-1), labels.reshape(-1)
    h = ref.height(V, below).reshape(-1)
    for r, t in enumerate(T):
        pts = np.nonzero(lab == r)[0]
        assert len(pts) == t["points"] and pts[0] == t["first"] and lab[peak[r]] == r
        assert h[peak[r]] == h[pts].max() and peak[r] == pts[h[pts] == h[pts].max()][0]
        if t["neighbour"] >= 0:
            assert ref.height(t["saddle"], below) <= h[peak[r]]
            want = t["saddle"] - flat[peak[r]] if below else flat[peak[r]] - t["saddle"]
            assert t["depth"] == want
    # the regions are unions of basins
    regions = regions_ref.regions(V, iso, below=below, faces=faces)[0].reshape(-1)
    pairs = np.unique(np.stack([lab[lab >= 0], regions[lab >= 0]]), axis=1)
    assert pairs.shape[1] == len(T)


def test_signed_zeros_order_by_their_bits():
    V = _line([0.0, -0.0, 0.0, -0.0, 0.0])
    labels, B, s, raw, rounds = ref.basins(V, 0.0, 0.0)           # -0.0 >= 0.0: all inside; +0.0 is the higher
    assert raw == 3 and labels.reshape(-1).tolist() == [0, 0, 1, 1, 2] and s == 0
    assert np.all(B["depth"] == 0.0) and np.all(np.signbit(B["saddle"])) and B["neighbour"].tolist() == [1, 0, 1]
    labels, B, s, raw, rounds = ref.basins(V, 0.0, 0.5)
    assert len(B) == 1 and B["argMax"][0] == 0 and B["argMin"][0] == 1


def test_the_empty_lattice_and_no_inside_point():
    for V in (np.zeros((0, 3, 4), np.float32), np.full((2, 3, 4), np.nan, np.float32), np.full((2, 3, 4), -1.0, np.float32)):
        labels, B, s, raw, rounds = ref.basins(V, 0.0, 1.0)
        assert (s, raw, rounds, len(B)) == (0, 0, 0, 0) and np.all(labels == -1) and labels.shape == V.shape
    assert ref.BASIN.itemsize == 96 and ref.longest_chain(np.full((2, 3, 4), np.nan, np.float32), 0.0) == 0


def test_longest_chain_of_a_ramp():
    V = np.arange(1000, dtype=np.float32).reshape(1, 1, -1)
    assert ref.longest_chain(V, 0.0) == 999 and ref.longest_chain(V, 0.0, below=True) == 0
    assert ref.basins(V, 0.0, 0.0)[3] == 1
