"""The kernels of exa_hip_histogram (csrc/exa_histogram.hip), read from the gfx950 code object the build left in csrc/ (no GPU
needed): the unit exists and holds only the binning kernel and the range-only kernel, both without scratch and without
spilled registers, at a register count that leaves the memory-bound pass its full occupancy.  A missing object is a
failure: build() makes it."""
from test_isomesh_kernels import _kernels

OBJ = "exa_histogram.o"
KERNELS = ["histKernelILb1E", "histKernelILb0E"]            # histKernel<true> (bins), histKernel<false> (range only)


def test_histogram_unit_holds_its_kernels_for_gfx950():
    k = _kernels(OBJ)
    for want in KERNELS:
        assert sum(1 for name in k if want in name) == 1, (want, sorted(k))
    assert len(k) == len(KERNELS) and all("histKernel" in name for name in k), sorted(k)


def test_histogram_kernels_have_no_scratch_no_spills_and_full_occupancy():
    k = _kernels(OBJ)
    assert len(k) >= len(KERNELS)
    for name, (vgpr, scratch, vspill, sspill) in k.items():
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, vgpr, scratch, vspill, sspill)
        assert vgpr <= 64, (name, vgpr)


def test_other_units_are_unchanged_by_the_histogram_unit():
    # the histogram kernels live in their own unit: the probe and iso-mesh units hold only their own kernels
    for obj in ("exa_sample_f0.o", "exa_sample_f1.o", "exa_sample_f0e.o", "exa_isomesh.o"):
        assert not any("histKernel" in name for name in _kernels(obj)), obj
