"""exaRender --histogram: the CLI writes the histogram the binding's Renderer.histogram returns, one line `cells volume` per
bin, and reports the channel, the bins, the range and the counts by class; the default range is the channel's min..max, and a
constant field is refused."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from common import ROOT, Case
from owlexabrick_amd import scenes

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "owlexabrick_amd", "host", "exaRender")


@pytest.mark.parametrize("how", ["default-range", "range-and-box"])
def test_exarender_histogram_writes_the_bindings_counts(how):
    scene = scenes.amr(levels=3, fields=2)
    R = Case(scene).hip_renderer()
    if how == "default-range":
        channel, bins, box, args = 0, 128, None, []
        st = R.fieldStats(channel)
        lo, hi = st["min"], st["max"]
    else:
        channel, bins, box = 1, 37, [1, 3, 1, 47, 45, 31]
        lo, hi = np.float32(0.3), np.float32(0.6)
        args = ["--histogram-channel", "1", "--histogram-range", repr(float(lo)), repr(float(hi)), "--histogram-box", *map(str, box)]
    cells, volume, st = R.histogram(channel, lo, hi, bins, box=box)
    assert st["binned"] > 0 and (how == "default-range" or (st["under"] > 0 and st["over"] > 0 and st["slots"] < scene.num_cells))
    with tempfile.TemporaryDirectory() as d:
        cfg = scenes.write_exa(scene, d, "amr")
        out = os.path.join(d, "hist.txt")
        r = subprocess.run([EXE, cfg, "--histogram", str(bins), out, "--frames", "0", *args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        got = np.loadtxt(out, dtype=np.uint64, ndmin=2)
    assert got.shape == (bins, 2)
    assert np.array_equal(got[:, 0], cells) and np.array_equal(got[:, 1], volume)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("histogram ")]
    assert len(line) == 1, r.stdout
    m = re.fullmatch(r"histogram channel (\d+) bins (\d+) range (\S+) (\S+) slots (\d+) empty (\d+) nan (\d+) under (\d+) over (\d+) "
                     r"binned (\d+)", line[0])
    assert m, line[0]
    assert (int(m.group(1)), int(m.group(2))) == (channel, bins)
    assert np.float32(m.group(3)) == lo and np.float32(m.group(4)) == hi             # %.9g round-trips a float32
    assert [int(m.group(k)) for k in range(5, 11)] == [st[k] for k in ("slots", "empty", "nan", "under", "over", "binned")]
    assert "Avg. after" not in r.stdout                        # --frames 0: nothing rendered
    R.close()


def test_exarender_histogram_refuses_a_constant_field_without_a_range():
    scene = scenes.example("ex3")
    scene.fields.append(np.full_like(scene.fields[0], 0.5))
    with tempfile.TemporaryDirectory() as d:
        cfg = scenes.write_exa(scene, d, "ex3")
        out = os.path.join(d, "hist.txt")
        r = subprocess.run([EXE, cfg, "--histogram", "16", out, "--histogram-channel", "1", "--frames", "0"], capture_output=True,
                           text=True, timeout=300)
        assert r.returncode != 0 and "constant" in r.stderr and "--histogram-range" in r.stderr, (r.stdout, r.stderr)
        assert not os.path.exists(out)
