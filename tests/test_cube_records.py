"""The 16-byte cube records of the one-channel rope march (owlexabrick_amd/csrc/exa_cube.h), on the CPU through the
diagnostic entry point exa_prep_cube_records: the packing of the record word, the float the kernel forms from it, the
records of a prepared scene, and every condition under which a scene is no cube scene (nothing is built then and the
march reads the 32-byte march headers, as before)."""
import numpy as np
import pytest

from owlexabrick_amd import binding, scenes

u32 = np.uint32


def bricks_of(rows):
    """BRICK_DTYPE array of (lower, size, level, begin) rows"""
    b = np.zeros(len(rows), dtype=binding.BRICK_DTYPE)
    for i, (lower, size, level, begin) in enumerate(rows):
        b[i] = (lower, size, level, begin)
    return b


def cube_scene(k, levels_begins, lower=(0, 0, 0)):
    S = 1 << k
    return bricks_of([(lower, (S, S, S), lv, index << (3 * k)) for lv, index in levels_begins])


def unpack(w, k):
    """(begin, level, float bits of 2^-level) as the kernel takes them from the record word"""
    w = int(w)
    return (w >> 9) << (3 * k), 127 - (w & 0x1FF), (w << 23) & 0xFFFFFFFF


@pytest.mark.parametrize("k", range(1, 8))
def test_record_word_round_trips_and_is_the_float(k):
    """k = 1..7, levels 0..30, index 0 and 2^23 - 1 (beyond k = 3 the largest index whose 32-bit begin exists, 2^(32-3k) - 1):
    begin and level come back, bit 8 is clear, and w << 23 is ldexpf(1, -level) bit for bit"""
    top = min((1 << 23) - 1, ((1 << 32) >> (3 * k)) - 1)
    assert top == (1 << 23) - 1 or k > 3
    indices = [0, 1, top]
    rows = [(lv, i) for lv in range(31) for i in indices]
    b = cube_scene(k, rows)
    got_k, rec = binding.cube_records(b, np.arange(len(b), dtype=np.int32))
    assert got_k == k and rec.shape == (len(b), 4)
    for (lv, i), r in zip(rows, rec):
        begin, level, fbits = unpack(r[3], k)
        assert begin == i << (3 * k) and level == lv and not (int(r[3]) >> 8) & 1, (lv, i, hex(int(r[3])))
        want = np.ldexp(np.float32(1), -lv).astype(np.float32)
        assert want.dtype == np.float32 and fbits == int(want.view(u32)), (lv, hex(fbits))


def test_lower_is_the_march_headers_float_and_the_records_follow_the_leaf_list():
    """x, y, z = float(lower) as float bits (negative and beyond-2^24 coordinates round as the conversion does); a brick listed
    twice and out of order gets its record at each place"""
    S = 4
    b = bricks_of([((-8, 0, 16777217), (S, S, S), 2, 0), ((4, -12, 8), (S, S, S), 0, 64), ((0, 0, 0), (S, S, S), 30, 128)])
    leaf = np.array([2, 0, 1, 0], dtype=np.int32)
    k, rec = binding.cube_records(b, leaf)
    assert k == 2
    for at, i in enumerate(leaf):
        assert np.array_equal(rec[at, :3], b["lower"][i].astype(np.float32).view(u32))
        assert unpack(rec[at, 3], k)[:2] == (int(b["begin"][i]), int(b["level"][i]))


def test_a_prepared_amr_scene_is_a_cube_scene_in_both_brick_orders():
    for B, k in ((2, 1), (4, 2), (8, 3)):
        prep = binding.Prep(scenes.amr(B=B, levels=3, root=(2, 2, 1)))
        b, leaf = prep.bricks(), prep.leaflist()
        got, rec = binding.cube_records(b, leaf, begin_alt=b["begin"][::-1].copy())     # any permutation of whole cubes
        assert got == k and len(rec) == len(leaf) > 0
        assert [unpack(w, k)[0] for w in rec[:, 3]] == [int(b["begin"][i]) for i in leaf]
        assert [unpack(w, k)[1] for w in rec[:, 3]] == [int(b["level"][i]) for i in leaf]
        assert np.array_equal(rec[:, :3], b["lower"][leaf].astype(np.float32).view(u32))
        prep.close()


REFUSED = {
    "mixed sizes": bricks_of([((0, 0, 0), (4, 4, 4), 0, 0), ((4, 0, 0), (4, 4, 2), 0, 64)]),
    "mixed cubes": bricks_of([((0, 0, 0), (4, 4, 4), 0, 0), ((4, 0, 0), (8, 8, 8), 0, 512)]),
    "edge 6": bricks_of([((0, 0, 0), (6, 6, 6), 0, 0), ((6, 0, 0), (6, 6, 6), 0, 216)]),
    "edge 1": bricks_of([((0, 0, 0), (1, 1, 1), 0, 0), ((1, 0, 0), (1, 1, 1), 0, 1)]),
    "edge 256": bricks_of([((0, 0, 0), (256, 256, 256), 0, 0)]),
    "begin no multiple of S^3": bricks_of([((0, 0, 0), (4, 4, 4), 0, 0), ((4, 0, 0), (4, 4, 4), 0, 65)]),
    "index 2^23": cube_scene(1, [(0, 0), (0, 1 << 23)]),
    "level 31": cube_scene(2, [(0, 0), (31, 1)]),
}


@pytest.mark.parametrize("why", sorted(REFUSED))
def test_scene_is_no_cube_scene(why):
    b = REFUSED[why]
    k, rec = binding.cube_records(b, np.arange(len(b), dtype=np.int32))
    assert k == 0 and rec is None


def test_the_other_brick_order_is_held_to_the_same_conditions():
    b = cube_scene(2, [(0, 0), (1, 1), (0, 2)])
    leaf = np.arange(3, dtype=np.int32)
    assert binding.cube_records(b, leaf)[0] == 2
    assert binding.cube_records(b, leaf, begin_alt=np.array([128, 0, 64], dtype=u32))[0] == 2
    assert binding.cube_records(b, leaf, begin_alt=np.array([128, 0, 65], dtype=u32))[0] == 0           # no multiple
    assert binding.cube_records(cube_scene(1, [(0, 0), (0, 1)]), leaf[:2], begin_alt=np.array([0, 8 << 23], dtype=u32))[0] == 0   # index 2^23


def test_the_largest_index_is_accepted_next_to_the_refused_one():
    b = cube_scene(1, [(0, 0), (0, (1 << 23) - 1)])
    k, rec = binding.cube_records(b, np.arange(2, dtype=np.int32))
    assert k == 1 and unpack(rec[1, 3], 1)[0] == ((1 << 23) - 1) << 3


def test_a_leaf_list_entry_out_of_range_is_an_error():
    b = cube_scene(2, [(0, 0)])
    with pytest.raises(RuntimeError, match="out of range"):
        binding.cube_records(b, np.array([1], dtype=np.int32))
