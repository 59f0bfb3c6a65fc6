"""exaRender --profile: the file holds the arrays and the counts that the binding's Renderer.profile returns for the same
arguments, byte for byte — one axis, two axes, --profile-log, --profile-weight, and `regions` / `basins` as the axis in one
invocation with --regions / --basins; its flag errors word for word, which fire before the config is read (no GPU)."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from common import ROOT, Case
from owlexabrick_amd import binding, scenes
from owlexabrick_amd.binding import channel, coordinate, derived, radius

EXE = os.path.join(ROOT, "owlexabrick_amd", "host", "exaRender")
DIMS = (23, 19, 17)
HEAD = (r"profile (\d+) (\d+) (\d+) bins (\d+) (\d+) values (\d+) weighted ([01]) points (\d+) outside (\d+) invalid (\d+) under (\d+) (\d+) "
        r"over (\d+) (\d+) binned (\d+) weightExponent (-?\d+) valueExponents (-?\d+) (-?\d+) (-?\d+) (-?\d+)")


def _read(path):
    """the .profile format: one text line, then count, the weight's sums, the sums, the minima and the maxima"""
    with open(path, "rb") as f:
        head = f.readline().decode()
        body = f.read()
    m = re.fullmatch(HEAD + "\n", head)
    assert m, head
    g = [int(x) for x in m.groups()]
    assert tuple(g[:3]) == DIMS
    B, nv, weighted = g[3] * g[4], g[5], g[6]
    at = [0]

    def take(dtype, n):
        a = np.frombuffer(body, dtype=dtype, count=n, offset=at[0])
        at[0] += a.nbytes
        return a
    out = dict(count=take(np.uint64, B), sum_weight=take(np.int64, B) if weighted else None, sums=take(np.int64, nv * B),
               mins=take(np.float32, nv * B), maxs=take(np.float32, nv * B))
    assert at[0] == len(body)
    out["stats"] = dict(points=g[7], outside=g[8], invalid=g[9], under=g[10:12], over=g[12:14], binned=g[14], weightExponent=g[15],
                        valueExponent=g[16:20])
    return out, head.strip()


def _same(got, want):
    for k in ("count", "sum_weight", "sums", "mins", "maxs"):
        if want[k] is None:
            assert got[k] is None, k
        else:
            assert got[k].tobytes() == want[k].tobytes(), k
    assert got["stats"] == {k: v for k, v in want["stats"].items() if k != "ldsTable"}


@pytest.mark.gpu
def test_exarender_profile_writes_the_bindings_bytes():
    scene = scenes.example("ex3")
    R = Case(scene).hip_renderer()
    lo, hi = (np.asarray(b, np.float64) for b in R.prep.voxel_bounds())
    ext = hi - lo
    box = [np.float32(v) for v in (lo - 0.1 * ext, hi + 0.05 * ext)]
    V = R.resample(*box, DIMS, fill=float("nan"))
    fin = V[np.isfinite(V)]
    a, b = float(fin.min()), float(fin.max())
    assert a < b and b > 0 and np.isnan(V).any()
    la = a if a > 0 else 0.001 * b                                  # --profile-log wants a positive range
    iso = float(np.float32(np.median(fin)))
    centre = (1.5, 2.25, 3.0)
    f = lambda x: repr(float(np.float32(x)))                       # noqa: E731
    rmax = float(np.float32(np.linalg.norm(ext)))
    log_edges = lambda lo_, hi_, n: np.array([np.float32(float(np.float32(lo_)) * (float(np.float32(hi_)) / float(np.float32(lo_))) ** (k / n))      # noqa: E731
                                              for k in range(n + 1)], np.float32)
    regions = R.regions(*box, DIMS, iso)
    basins = R.basins(*box, DIMS, iso, 0.0625)
    assert len(regions["regions"]) > 0 and len(basins["basins"]) > 0
    cases = [
        ([f"c0@{f(a)}:{f(b)}:16", "c0+x"], [],
         lambda: R.profile(*box, DIMS, binding.uniform(channel(0), a, b, 16), [channel(0), coordinate(0)])),
        ([f"r:1.5,2.25,3@0:{f(rmax)}:8/c0@{f(a)}:{f(b)}:5", "q:0,0,0+c0"], ["--profile-weight", "z"],
         lambda: R.profile(*box, DIMS, [binding.uniform(radius(centre), 0.0, rmax, 8), binding.uniform(channel(0), a, b, 5)],
                           [derived("q", (0, 0, 0)), channel(0)], coordinate(2))),
        ([f"c0@{f(la)}:{f(b)}:12", "none"], ["--profile-log"],
         lambda: R.profile(*box, DIMS, binding.edges(channel(0), log_edges(la, b, 12)))),
        (["regions", "c0"], ["--regions", "0", repr(iso), *map(str, DIMS), "REGIONS"],
         lambda: R.profile(*box, DIMS, binding.labels(regions["labels"], len(regions["regions"])), [channel(0)])),
        (["basins/y@-100:100:3", "c0"], ["--basins", "0", repr(iso), "0.0625", *map(str, DIMS), "BASINS"],
         lambda: R.profile(*box, DIMS, [binding.labels(basins["labels"], len(basins["basins"])), binding.uniform(coordinate(1), -100.0, 100.0, 3)],
                           [channel(0)])),
    ]
    boxargs = [repr(float(c)) for v in box for c in v]
    with tempfile.TemporaryDirectory() as d:
        cfg = scenes.write_exa(scene, d, "ex3")
        out = os.path.join(d, "out.profile")
        for words, extra, call in cases:
            extra = [os.path.join(d, w) if w in ("REGIONS", "BASINS") else w for w in extra]
            lattice_flags = ["--regions-box", *boxargs] if extra and extra[0] in ("--regions", "--basins") else []
            r = subprocess.run([EXE, cfg, "--frames", "0", "--profile", *words, *map(str, DIMS), out, "--profile-box", *boxargs, *extra,
                                *lattice_flags], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, (words, r.stderr)
            got, head = _read(out)
            want = call()
            assert want["stats"]["binned"] > 0, words
            _same(got, want)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("profile ")]
            assert line == [f"{head} world 0 log {1 if '--profile-log' in extra else 0} lds {want['stats']['ldsTable']}"], r.stdout
            assert "Avg. after" not in r.stdout                    # --frames 0: nothing rendered
        # the regions' own file of the combined invocation is what --regions alone writes: the labels the profile read
        r = subprocess.run([EXE, cfg, "--frames", "0", "--profile", "regions", "c0", *map(str, DIMS), out, "--regions", "0", repr(iso),
                            *map(str, DIMS), out + ".r"], capture_output=True, text=True, timeout=300)      # neither has a box: the same lattice
        assert r.returncode == 0 and r.stdout.index("\nregions ") < r.stdout.index("\nprofile "), (r.stdout, r.stderr)
        r = subprocess.run([EXE, cfg, "--frames", "0", "--profile", "c0@0:1:4", "vorticity:0,0,0", *map(str, DIMS), out], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode != 0 and "exa_hip_profile" in r.stderr + r.stdout and "one-component" in r.stderr + r.stdout
    R.close()


SOURCE = "--profile wants a source cN, QUANTITY:C0,C1,C2, r:x,y,z, x, y or z, not "
AXIS = "--profile wants an axis SOURCE@LO:HI:BINS, regions or basins, not "
LOG = "--profile-log wants edges LO * (HI / LO)^(b / BINS) that ascend strictly (0 < LO < HI, BINS >= 1 and not too many)"
TAIL = ["2", "2", "2", "o.profile"]
TABLE = [
    (["--profile"], "missing axes after --profile"),
    (["--profile", "c0@0:1:4"], "missing values after --profile AXIS[/AXIS]"),
    (["--profile", "c0@0:1:4", "none", "2", "2"], "missing value after --profile"),
    (["--profile", "c0@0:1:4", "none", "2", "2", "2"], "missing file after --profile AXIS[/AXIS] VALUES NX NY NZ"),
    (["--profile-weight"], "missing source after --profile-weight"),
    (["--profile-box", "0", "0", "0", "1", "1"], "missing value after --profile-box"),
    (["--profile", "c0@0:1:4/c0@0:1:4/x@0:1:2", "none", *TAIL], "--profile wants one or two axes AXIS[/AXIS]"),
    (["--profile", "c0@0:1", "none", *TAIL], AXIS + "c0@0:1"),
    (["--profile", "c0", "none", *TAIL], AXIS + "c0"),
    (["--profile", "c0@0:1:4x", "none", *TAIL], AXIS + "c0@0:1:4x"),
    (["--profile", "q@0:1:4", "none", *TAIL], SOURCE + "q"),
    (["--profile", "c0@0:1:4", "c", *TAIL], SOURCE + "c"),
    (["--profile", "c0@0:1:4", "c0+", *TAIL], SOURCE),
    (["--profile", "c0@0:1:4", "q:0,1", *TAIL], SOURCE + "q:0,1"),
    (["--profile", "c0@0:1:4", "r:1,2", *TAIL], SOURCE + "r:1,2"),
    (["--profile", "c0@0:1:4", "w", *TAIL], SOURCE + "w"),
    (["--profile", "c0@0:1:4", "bogus:0,1,2", *TAIL],
     "--derived wants speed, divergence, vorticity, vorticity_magnitude, q, helicity or a number, not bogus"),
    (["--profile", "c0@0:1:4", "none", *TAIL, "--profile-weight", "c1x"], SOURCE + "c1x"),
    (["--profile", "c0@0:1:4", "c0+c0+c0+c0+c0", *TAIL], "--profile wants at most 4 values"),
    (["--profile", "c0@0:1:4/regions", "none", *TAIL], "--profile takes regions as its first axis only"),
    (["--profile", "c0@0:1:4/basins", "none", *TAIL], "--profile takes basins as its first axis only"),
    (["--profile", "regions", "none", *TAIL], "--profile regions needs --regions on the same lattice in the same invocation"),
    (["--profile", "basins", "none", *TAIL], "--profile basins needs --basins on the same lattice in the same invocation"),
    (["--profile", "regions", "none", *TAIL, "--regions", "0", "0.5", "2", "2", "3", "r"],
     "--profile regions needs --regions on the same lattice in the same invocation"),
    (["--profile", "regions", "none", *TAIL, "--regions", "0", "0.5", "2", "2", "2", "r", "--profile-world"],
     "--profile regions needs --regions on the same lattice in the same invocation"),
    (["--profile", "regions", "none", *TAIL, "--regions", "0", "0.5", "2", "2", "2", "r", "--regions-box", "0", "0", "0", "1", "1", "1"],
     "--profile regions needs --regions on the same lattice in the same invocation"),
    (["--profile", "basins", "none", *TAIL, "--regions", "0", "0.5", "2", "2", "2", "r"],
     "--profile basins needs --basins on the same lattice in the same invocation"),
    (["--profile", "c0@0:1:4", "none", *TAIL, "--profile-log"], LOG),
    (["--profile", "c0@2:1:4", "none", *TAIL, "--profile-log"], LOG),
    (["--profile", "c0@1:1.0000001:64", "none", *TAIL, "--profile-log"], LOG),
]


@pytest.mark.parametrize("args,text", TABLE, ids=[" ".join(a)[:60] for a, _ in TABLE])
def test_profile_flag_errors_word_for_word(args, text):
    r = subprocess.run([EXE, "no_such_config.exa", *args], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    last = (r.stderr + r.stdout).strip().splitlines()[-1]
    assert last.endswith(text.strip()), (args, last)
