"""exaRender with every analysis output in one invocation: each file is, byte for byte, the file of an invocation that asks for
that output alone, and stdout holds the same result lines in the documented order.  What the outputs share is pinned this way:
--derived (resample, isomesh, isolines, regions, basins), the --regions-* flags (regions and basins), the --size image (project,
raycast) and the mesh that --isomesh leaves on the device for --surface iso."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from common import ROOT
from owlexabrick_amd import scenes

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "owlexabrick_amd", "host", "exaRender")
LATTICE = ["9", "8", "7"]
PLANE = ["0", "0", "2", repr(8 / 11), "0", "0", "0", repr(8 / 9), "0", "11", "9"]     # the slice z = 2 of ex3's 8 x 8 x 4 voxels
BOX = ["1", "1", "0.5", "7", "7", "3.5"]
ORDER = ["resample", "isomesh", "isolines", "lic", "ftle", "critical", "regions", "basins", "surface", "histogram", "streamlines",
         "project", "raycast"]


def _count(line, word):
    words = line.split()
    return int(words[words.index(word) + 1])


def test_all_outputs_at_once_equal_each_alone():
    scene = scenes.example("ex3")
    with tempfile.TemporaryDirectory() as d:
        cfg = scenes.write_exa(scene, d, "ex3")
        seeds = os.path.join(d, "seeds.txt")
        with open(seeds, "w") as f:
            f.write("2 2 1\n4 4 2\n6 5 3\n")
        common = [cfg, "--size", "16", "12", "--frames", "0", "--derived", "q", "0", "0", "0"]

        def run(tag, flags):
            """the flags with every `@name` replaced by the file tag_name; stdout's lines and the files' bytes"""
            names = {a[1:]: os.path.join(d, f"{tag}_{a[1:]}") for a in flags if a.startswith("@")}
            r = subprocess.run([EXE] + common + [names[a[1:]] if a.startswith("@") else a for a in flags],
                               capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, (tag, r.stderr)
            assert "Avg. after" not in r.stdout                         # --frames 0: nothing rendered
            return r.stdout.splitlines(), {k: open(p, "rb").read() for k, p in names.items()}

        # the resampled quantity gives the level that the lattice outputs cut it at: its median
        flags = {"resample": ["--resample", *LATTICE, "@resample"]}
        lines, files = run("one", flags["resample"])
        single = {"resample": (lines, files)}
        q = np.frombuffer(files["resample"], dtype=np.float32)
        assert q.size == 9 * 8 * 7
        iso = repr(float(np.float32(np.median(q[np.isfinite(q)]))))
        lattice = ["--regions-box", *BOX, "--regions-below"]
        isomesh = ["--isomesh", iso, *LATTICE, "@isomesh"]
        flags.update({
            "isomesh": isomesh,
            "isolines": ["--isolines", "0", *PLANE, iso + "," + repr(float(iso) / 2), "@isolines"],
            "lic": ["--lic", "0,0,0", *PLANE, "0.5", "6", "@lic", "--lic-seed", "7"],
            "ftle": ["--ftle", "0,0,0", *BOX, *LATTICE, "0.25", "8", "fwd", "@ftle"],
            "critical": ["--critical", "0,0,0", *BOX, *LATTICE, "8", "0.001", "@critical"],
            "regions": ["--regions", "0", iso, *LATTICE, "@regions", *lattice],
            "basins": ["--basins", "0", iso, "0.0625", *LATTICE, "@basins", *lattice],
            "surface": [*isomesh, "--surface", "iso", "0", "0.5", "4", "@surface"],      # iso: the mesh of this invocation
            "histogram": ["--histogram", "8", "@histogram"],
            "streamlines": ["--streamlines", seeds, "0.25", "16", "@streamlines", "--streamlines-channels", "0", "0", "0"],
            "project": ["--project", "0", "0.5", "32", "@project"],
            "raycast": ["--raycast", "0", "0.4", "0.5", "32", "4", "@raycast"],
        })
        for name in ORDER[1:]:
            single[name] = run("one", flags[name])
        every = [a for name in ORDER if name != "isomesh" for a in flags[name]]     # the surface's flags hold the isomesh's
        lines, files = run("all", every)

    assert sorted(files) == sorted(ORDER)
    for name in ORDER:
        assert files[name] == single[name][1][name], name
        assert len(files[name]) > 0, name
    # stdout: what precedes the outputs (config, camera), then one line per output, each the last line of its own invocation
    head = single["resample"][0][:-1]
    assert head[-1].startswith("camera ") and lines[:len(head)] == head
    results = lines[len(head):]
    assert [line.split()[0] for line in results] == ORDER
    assert results == [single[name][0][-1] for name in ORDER]
    for name in ORDER:
        assert single[name][0][:len(head)] == head, name
    by = dict(zip(ORDER, results))
    assert " derived 4 channels 0 0 0 " in by["basins"] and " below 1 " in by["basins"] and " below 1 " in by["regions"]
    # nothing is empty at these sizes (critical points are a matter of the scene: its line is compared above)
    assert _count(by["isomesh"], "triangles") > 0 and _count(by["isolines"], "segments") > 0
    assert _count(by["regions"], "count") > 0 and _count(by["basins"], "count") > 0
    assert _count(by["surface"], "triangles") == _count(by["isomesh"], "triangles")
    # the basins went by --regions-box and --regions-below: their inside points are the regions' (include/exa_hip.h: the same test)
    assert 0 < _count(by["basins"], "inside") == _count(by["regions"], "inside") < 9 * 8 * 7
