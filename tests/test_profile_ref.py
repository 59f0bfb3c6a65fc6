"""tests/profile_ref.py, the numpy restatement of exa_hip_profile's contract, against a plain loop over the points that follows
include/exa_hip.h sentence by sentence; the exponent rule and the rounding at their edges.  No GPU."""
import math
import struct
import warnings

import numpy as np
import pytest

import profile_ref as ref

F = np.float32
FLT_MAX = float(np.finfo(F).max)


def _key(v):
    b = struct.unpack("<I", struct.pack("<f", float(v)))[0]
    return (~b & 0xffffffff) if b >> 31 else (b | 0x80000000)


def _q(v, s):
    x = math.ldexp(float(v), s)                 # exact in double for these exponents
    r = math.floor(x)
    d = x - r
    if d > 0.5 or (d == 0.5 and r % 2):
        r += 1
    return int(r)


def _exp(terms):
    M = max((abs(float(t)) for t in terms), default=0.0)
    return 0 if M == 0.0 else 30 - math.frexp(M)[1]


def loop_profile(axes, values, weight):
    """the contract point by point: classes in order, the bin, then the sums with the exponents of the binned terms"""
    n = len(axes[0]["lab"] if axes[0]["mode"] == "labels" else axes[0]["v"])
    B = int(np.prod([a["n"] for a in axes]))
    st = dict(points=n, outside=0, invalid=0, under=[0, 0], over=[0, 0], binned=0)
    rows = []                                   # (bin, w, [v], [term]) of the binned points
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for L in range(n):
            if axes[0]["mode"] == "labels" and axes[0]["lab"][L] < 0:
                st["outside"] += 1
                continue
            keys = [None if a["mode"] == "labels" else F(a["v"][L]) for a in axes]
            w = None if weight is None else F(weight[L])
            vs = [F(v[L]) for v in values]
            terms = [v if w is None else F(w * v) for v in vs]
            if any(k is not None and math.isnan(k) for k in keys) or not all(math.isfinite(x) for x in vs + terms + ([w] if w is not None else [])):
                st["invalid"] += 1
                continue
            b, stride, out = 0, 1, False
            for k, (a, x) in enumerate(zip(axes, keys)):
                if a["mode"] == "labels":
                    bk = int(a["lab"][L])
                else:
                    lo, hi = (a["lo"], a["hi"]) if a["mode"] == "uniform" else (a["e"][0], a["e"][-1])
                    if x < lo:
                        st["under"][k] += 1
                        out = True
                        break
                    if x > hi:
                        st["over"][k] += 1
                        out = True
                        break
                    if a["mode"] == "uniform":
                        t = F(F(x - lo) * F(F(a["n"]) / F(hi - lo)))
                        bk = min(a["n"] - 1, int(t))
                    else:
                        bk = a["n"] - 1 if x == a["e"][-1] else max(i for i in range(a["n"]) if a["e"][i] <= x)
                b += bk * stride
                stride *= a["n"]
            if out:
                continue
            st["binned"] += 1
            rows.append((b, w, vs, terms))
    count = np.zeros(B, np.uint64)
    sw = None if weight is None else np.zeros(B, np.int64)
    sums = np.zeros((len(values), B), np.int64)
    mins, maxs = np.full((len(values), B), np.inf, F), np.full((len(values), B), -np.inf, F)
    st["weightExponent"] = _exp([r[1] for r in rows]) if weight is not None else 0
    st["valueExponent"] = [_exp([r[3][f] for r in rows]) if f < len(values) else 0 for f in range(4)]
    kmin, kmax = {}, {}
    for b, w, vs, terms in rows:
        count[b] += 1
        if w is not None:
            sw[b] += _q(w, st["weightExponent"])
        for f, (v, t) in enumerate(zip(vs, terms)):
            sums[f, b] += _q(t, st["valueExponent"][f])
            if (f, b) not in kmin or _key(v) < _key(kmin[f, b]):
                kmin[f, b] = v
            if (f, b) not in kmax or _key(v) > _key(kmax[f, b]):
                kmax[f, b] = v
    for (f, b), v in kmin.items():
        mins[f, b] = v
    for (f, b), v in kmax.items():
        maxs[f, b] = v
    return dict(count=count, sum_weight=sw, sums=sums, mins=mins, maxs=maxs, stats=st)


def same(got, want):
    for k in ("count", "sum_weight", "sums", "mins", "maxs"):
        if want[k] is None:
            assert got[k] is None, k
        else:
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])
    assert got["stats"] == want["stats"], (got["stats"], want["stats"])


SPECIAL = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, 2.0, 3.0, -1.0, 3e38, -3e38, 1e-40]


def field(rng, n, scale=1.0, special=0.15):
    v = (rng.standard_normal(n) * scale).astype(F)
    at = rng.random(n) < special
    v[at] = rng.choice(np.array(SPECIAL, F), int(at.sum()))
    return v


@pytest.mark.parametrize("seed", range(4))
def test_restatement_against_the_loop_one_axis(seed):
    rng = np.random.default_rng(seed)
    n = 300
    key, a, b, w = field(rng, n, 2.0), field(rng, n), field(rng, n, 1e3), field(rng, n, 1.0, 0.05)
    key[:8] = [-1.0, 3.0, 1.0, 2.0, 0.0, -0.0, 2.9999998, -1.0000001]           # lo, hi, the edges, and next to them
    w[rng.random(n) < 0.3] *= F(-1)
    for axis in (ref.uniform(key, -1.0, 3.0, 7), ref.edges(key, [-1.0, 0.0, 1.0, 2.0, 3.0]), ref.uniform(key, 0.0, 1.0, 1)):
        same(ref.profile([axis], [a, b], w), loop_profile([axis], [a, b], w))
        same(ref.profile([axis], [a, b, a]), loop_profile([axis], [a, b, a], None))
        same(ref.profile([axis]), loop_profile([axis], [], None))
    got = ref.profile([ref.uniform(key, -1.0, 3.0, 7)], [a, b], w)
    assert got["stats"]["invalid"] > 0 and got["stats"]["under"][0] > 0 and got["stats"]["over"][0] > 0 and got["stats"]["binned"] > 0


@pytest.mark.parametrize("seed", range(3))
def test_restatement_against_the_loop_two_axes_and_labels(seed):
    rng = np.random.default_rng(100 + seed)
    n = 400
    k0, k1, a, w = field(rng, n, 2.0), field(rng, n, 2.0), field(rng, n), field(rng, n, 1.0, 0.05)
    lab = rng.integers(-2, 6, n).astype(np.int32)
    pairs = [[ref.uniform(k0, -2.0, 2.0, 7), ref.edges(k1, [-3.0, -0.5, 0.0, 0.25, 1.0, 8.0])],
             [ref.labels(lab, 6), ref.uniform(k1, -1.0, 1.0, 5)],
             [ref.labels(lab, 6)],
             [ref.labels(np.full(n, -1, np.int32), 3)]]
    for axes in pairs:
        same(ref.profile(axes, [a], w), loop_profile(axes, [a], w))
        same(ref.profile(axes, [a, k0]), loop_profile(axes, [a, k0], None))
    two = ref.profile(pairs[0], [a], w)["stats"]
    assert two["under"][1] + two["over"][1] > 0
    none = ref.profile(pairs[3], [a], w)
    assert none["stats"]["binned"] == 0 and none["stats"]["outside"] == n and none["stats"]["valueExponent"] == [0, 0, 0, 0]
    assert np.isposinf(none["mins"]).all() and np.isneginf(none["maxs"]).all()


def test_a_label_beyond_the_bins_is_refused_with_the_first_index():
    lab = np.array([0, 1, 5, 2, 7], np.int32)
    with pytest.raises(ValueError, match="first at L = 2"):
        ref.profile([ref.labels(lab, 5)])


def test_an_overflowing_product_is_invalid_and_a_negative_weight_is_not():
    key = np.zeros(4, F)
    v = np.array([3e38, 1.0, -3e38, 2.0], F)
    w = np.array([2.0, -2.0, 2.0, 0.5], F)
    got = ref.profile([ref.uniform(key, -1.0, 1.0, 2)], [v], w)
    assert got["stats"]["invalid"] == 2 and got["stats"]["binned"] == 2
    s = got["stats"]["valueExponent"][0]
    assert got["sums"][0].sum() == round(math.ldexp(-2.0 + 1.0, s)) and got["sum_weight"].sum() == round(math.ldexp(-1.5, got["stats"]["weightExponent"]))


@pytest.mark.parametrize("M,want", [(0.0, 0), (1.0, 29), (0.75, 30), (1e-45, 30 + 148), (1.1754944e-38, 30 + 125), (FLT_MAX, 30 - 128)])
def test_exponent_edge_cases(M, want):
    key = np.zeros(3, F)
    v = np.array([M, -M, 0.0], F)
    got = ref.profile([ref.uniform(key, -1.0, 1.0, 1)], [v])
    assert got["stats"]["valueExponent"][0] == want
    if M:
        q = int(got["sums"][0][0])
        assert q == 0 and abs(int(ref.quantised(F(M), want))) in range(1 << 29, (1 << 30) + 1)     # |q(M)| in [2^29, 2^30]


def test_no_binned_point_gives_exponent_zero():
    key = np.full(5, 9.0, F)
    got = ref.profile([ref.uniform(key, 0.0, 1.0, 4)], [np.ones(5, F)], np.ones(5, F))
    assert got["stats"]["binned"] == 0 and got["stats"]["over"][0] == 5
    assert got["stats"]["weightExponent"] == 0 and got["stats"]["valueExponent"] == [0, 0, 0, 0] and not got["count"].any()


def test_rint_ties_go_to_even():
    # M = 2^30 has e = 31: s = -1, and the odd integers below it sit on ties
    key = np.zeros(5, F)
    v = np.array([2.0 ** 30, 1.0, 3.0, 5.0, -3.0], F)
    got = ref.profile([ref.uniform(key, -1.0, 1.0, 1)], [v])
    assert got["stats"]["valueExponent"][0] == -1
    assert int(got["sums"][0][0]) == (1 << 29) + 0 + 2 + 2 - 2
    assert [int(x) for x in ref.quantised(np.array([0.5, 1.5, 2.5, -0.5, -1.5], F), 0)] == [0, 2, 2, 0, -2]
