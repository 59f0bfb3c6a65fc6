// exaRender — headless stand-in for the reference's exaViewer (exa/viewer.cpp): same config
// file, same camera / transfer-function / iso flags, same per-frame call sequence into the
// renderer, N frames instead of a GLUT loop, result written as binary PPM.
//   exaRender cfg.exa [--size W H] [--camera px py pz  ix iy iz  ux uy uz] [--fov deg]
//             [--dt f] [--xf file.xf] [--xf-scale s] [--range lo hi] [--isovals a b] [--isochans a b]
//             [--contourplane nx ny nz offset]... [--contourchan c]...   (exa/viewer.cpp:1199-1207, at most 3 planes)
//             [--clip-box lx ly lz ux uy uz] [--ao] [--ao-length l] [--no-pg] [--no-space-skipping]
//             [--gradientShadingDVR 0|1] [--gradientShadingISO 0|1] [--frames N] [-o out.ppm] [--info] [--stats]
//             [--gpus N | --devices 0,1,..]  one renderer over several GPUs (tiles dealt round-robin, stored straight into
//                                            the first device's frame); a device may be listed more than once
//             [--allow-empty-cells]          cell id -1 in the .bricks file = no cell (the reference's ALLOW_EMPTY_CELLS build)
//             [--option key=int]...          exa_hip_set_option, e.g. walk=1|2 (stack / rope walk of the region kd-tree), ao_overlap=0
//             [--pipeline]                   frames go to two device buffers in turn, frame k's copy to the host overlaps
//                                            frame k+1's march
//             [--resample NX NY NZ file.raw] the field on a uniform grid of cell centres (exa_hip_resample) as plain float32,
//                                            x fastest (the inverse of the reference's tools/fromVolume/raw2cells.cpp), with
//             [--resample-box lx ly lz ux uy uz] [--resample-world] [--resample-channel c] [--resample-fill v]
//                                            (box default: the voxel bounds, or the world bounds with --resample-world;
//                                            fill default NaN); --frames 0 renders nothing
//             [--isomesh ISO NX NY NZ file.tris] the iso-surface field == ISO on that lattice (exa_hip_isosurface: marching
//                                            tetrahedra, indexed, oriented toward the lower values) in the triangle file format
//                                            a config's `triangles` line reads, with
//             [--isomesh-box lx ly lz ux uy uz] [--isomesh-world] [--isomesh-channel c]
//                                            (box default as for --resample)
//             [--derived QUANTITY C0 C1 C2]  --resample and --isomesh work on a quantity of the velocity gradient tensor of the
//                                            vector field of channels C0 C1 C2 instead of a channel (exa_hip_resample_derived,
//                                            exa_hip_isosurface_derived; voxel-space quantities): speed, divergence, vorticity,
//                                            vorticity_magnitude, q or helicity, or its number 0..5.  vorticity has three
//                                            components, written interleaved by --resample and refused by --isomesh.  With it
//                                            --resample-channel / --isomesh-channel are an error
//             [--isolines CHANNEL ox oy oz ux uy uz vx vy vz NU NV ISO[,ISO...] out.isolines] the contour lines field == ISO of
//                                            CHANNEL, for every ISO of the list, on the plane lattice of NU x NV points whose
//                                            point (i,j) lies at o + (i + .5) u + (j + .5) v in voxel space (exa_hip_isolines:
//                                            marching triangles, indexed, the >= ISO side to the left of every segment).  With
//                                            --derived the lines of that quantity (exa_hip_isolines_derived; CHANNEL is read and
//                                            ignored, vorticity refused).  One text line `isolines NU NV levels N vertices V
//                                            segments S`, then raw little-endian arrays: the levels (N float32), vertexOffsets
//                                            and segmentOffsets (N + 1 uint64 each: level l owns the vertices / segments from
//                                            offset l up to offset l + 1), vertices (V x 3 float32, in the plane's space), uv
//                                            (V x 2 float32, lattice coordinates), segments (S x 2 int32, indices into the
//                                            vertices); --frames 0 renders nothing; with
//             [--isolines-world]             the plane is in world space
//             [--lic C0,C1,C2 ox oy oz ux uy uz vx vy vz NU NV STEP HALFLENGTH out.lic] line integral convolution of the vector
//                                            field of channels C0 C1 C2 on the plane lattice of --isolines, voxel space
//                                            (exa_hip_lic: per pixel the built-in noise along the field line of the in-plane
//                                            part, HALFLENGTH steps of STEP pixels backward and forward, averaged).  One text
//                                            line `lic NU NV channels C0 C1 C2 step STEP halfLength L seed N`, then the image:
//                                            NU*NV raw little-endian float32, row j = 0 first (NaN where the pixel's centre has
//                                            no value); --frames 0 renders nothing; with
//             [--lic-seed N]                 the seed of the built-in noise (default 0)
//             [--ftle C0,C1,C2 lx ly lz ux uy uz NX NY NZ STEP NUMSTEPS fwd|bwd out.ftle] flow map and FTLE of the vector field of
//                                            channels C0 C1 C2 on the lattice of --resample over the box [l, u], voxel space
//                                            (exa_hip_flowmap: NUMSTEPS RK4 steps of the time STEP from every lattice point,
//                                            forward or backward in time).  One text line `ftle NX NY NZ channels C0 C1 C2 step
//                                            STEP numSteps N direction fwd|bwd`, then five raw little-endian arrays, each in the
//                                            order (k*NY + j)*NX + i: end (3 float32 per point), steps (uint32), reasons (int32),
//                                            stretch (float32), ftle (float32; NaN where the point or a stencil neighbour did
//                                            not last the time); --frames 0 renders nothing
//             [--critical C0,C1,C2 lx ly lz ux uy uz NX NY NZ ITERATIONS TOLERANCE out.crit] the critical points of the vector
//                                            field of channels C0 C1 C2 on the lattice of --resample over the box [l, u], voxel
//                                            space (exa_hip_critical_points: the zeros of the trilinear interpolant, one per
//                                            cell at the most, by ITERATIONS Newton steps, accepted within TOLERANCE, classified
//                                            by the Jacobian).  One text line `critical NX NY NZ box lx ly lz ux uy uz channels
//                                            C0 C1 C2 iterations N tolerance T cells .. invalidCells .. candidates .. found ..
//                                            nonFinite .. leftCell .. notConverged ..`, then `found` raw little-endian records of
//                                            104 bytes (ExaHipCriticalPoint of include/exa_hip.h), in ascending cell number;
//                                            --frames 0 renders nothing
//             [--regions CHANNEL ISO NX NY NZ out.regions] the connected regions of field >= ISO of CHANNEL on that lattice
//                                            (exa_hip_regions: joined along the edges of --isomesh's tetrahedra, numbered by
//                                            their smallest lattice index, exact measurements per region).  With --derived the
//                                            regions of that quantity (exa_hip_regions_derived; CHANNEL is read and ignored,
//                                            vorticity refused).  One text line `regions NX NY NZ count R inside I exponent S`,
//                                            then raw little-endian arrays: the table (R records of 88 bytes, ExaHipRegion of
//                                            include/exa_hip.h: a region's value sum is sumFixed * 2^-S) and the labels
//                                            (NX*NY*NZ int32, x fastest: the region's number, -1 outside); --frames 0 renders
//                                            nothing; with
//             [--regions-box lx ly lz ux uy uz] [--regions-world] (box default as for --resample)
//             [--regions-below]              field < ISO instead
//             [--regions-faces]              joined along the three axes only (6 neighbours)
//             [--basins CHANNEL ISO MINDEPTH NX NY NZ out.basins] the basins of field >= ISO of CHANNEL on that lattice: one per
//                                            local maximum, those shallower than MINDEPTH (`inf` is allowed) merged across their
//                                            highest pass (exa_hip_basins).  With --derived the basins of that quantity
//                                            (exa_hip_basins_derived; CHANNEL is read and ignored, vorticity refused).  One text
//                                            line `basins NX NY NZ count B raw P rounds N inside I exponent S`, then raw
//                                            little-endian arrays: the table (B records of 96 bytes, ExaHipBasin of
//                                            include/exa_hip.h) and the labels (NX*NY*NZ int32, x fastest: the basin's number, -1
//                                            outside); --frames 0 renders nothing; --regions-box, --regions-world,
//                                            --regions-below and --regions-faces apply to it as well
//             [--profile AXIS[/AXIS] VALUES NX NY NZ out.profile] the points of that lattice binned by one or two axes, with the
//                                            count, the exact sums and the min / max of VALUES per bin (exa_hip_profile).
//                                            SOURCE is cN (channel N), QUANTITY:C0,C1,C2 (the names of --derived), r:x,y,z (the
//                                            distance from that centre) or x, y, z (a coordinate); AXIS is SOURCE@LO:HI:BINS
//                                            (uniform bins) or, as the first axis, the word regions or basins: the labels of
//                                            this invocation's --regions / --basins, which must be on the same lattice; VALUES
//                                            is up to four sources joined with +, or none.  One text line `profile NX NY NZ bins
//                                            B0 B1 values V weighted W points .. outside .. invalid .. under .. .. over .. ..
//                                            binned .. weightExponent .. valueExponents .. .. .. ..` (B1 = 1 with one axis),
//                                            then raw little-endian arrays over the B0*B1 bins, the first axis fastest: count
//                                            (uint64), with a weight its sums (int64), the V sums (int64: a sum is fixed *
//                                            2^-exponent), the V minima and the V maxima (float32); --frames 0 renders nothing; with
//             [--profile-weight SOURCE]      sums of weight * value, and the weight's own sums
//             [--profile-box lx ly lz ux uy uz] [--profile-world] (box default as for --resample)
//             [--profile-log]                the uniform axes' bins spaced logarithmically: edges float(LO * (HI / LO)^(b / BINS))
//             [--distance CHANNEL ISO MAXDIST NX NY NZ out.dist] per point of that lattice the exact Euclidean distance, in the
//                                            space of the box, to the nearest point where the field of CHANNEL is >= ISO, and
//                                            that point (exa_hip_distance; MAXDIST may be `inf`).  With
//                                            --derived the set of that quantity (exa_hip_distance_derived; CHANNEL is read and
//                                            ignored, vorticity refused).  One text line `distance NX NY NZ points P inside I
//                                            reached R maxDistance D`, then raw little-endian arrays over the lattice, x fastest:
//                                            dist (float32; +-inf beyond MAXDIST or with no target) and nearest (int32: the
//                                            linear index of the nearest target, -1 for none); --frames 0 renders nothing; with
//             [--distance-box lx ly lz ux uy uz] (box default as for --resample)
//             [--distance-signed]            + the distance to the set outside it, - the distance to the others inside it
//             [--distance-outside]           the distance to the nearest point that is not in the set (with ISO -3.4028235e38,
//                                            -FLT_MAX: the wall distance, to the nearest point without data)
//             [--histogram BINS file.txt]   the exact histogram of a channel's cell values (exa_hip_histogram), one line
//                                            `cells volume` per bin (cell slots; the same weighted with 8^level finest voxels), with
//             [--histogram-channel c] [--histogram-range lo hi] [--histogram-box lx ly lz ux uy uz]
//                                            (range default: min..max of the channel from a range-only pass — a constant field
//                                            is refused; box: integer voxel coordinates, default everything); --frames 0
//                                            renders nothing
//             [--streamlines SEEDS.txt STEP MAXSTEPS out.lines] field lines of three channels from the seeds of SEEDS.txt (one
//                                            `x y z` per line, voxel space) by fixed-step RK4 (exa_hip_streamlines); one text
//                                            line per polyline: `seedVertex backwardReason forwardReason count` and the
//                                            count vertices `x y z` (%.9g), with
//             [--streamlines-channels a b c] [--streamlines-both] [--streamlines-backward] [--streamlines-normalize]
//                                            (channels default 0 1 2; forward unless --streamlines-backward); --frames 0
//                                            renders nothing
//             [--project CHANNEL DT NSAMPLES out.prj] the field of CHANNEL reduced along the camera's rays through the pixel
//                                            centres of the --size image (exa_hip_project: world space, unit directions,
//                                            samples at (i + .5) * DT, i < NSAMPLES): one text line `project W H channel C dt
//                                            DT samples N`, then four raw little-endian planes of W x H, row y = 0 first:
//                                            the line integral sum*dt (float32), the number of valid samples (uint32), their
//                                            maximum and their minimum (float32; -inf / +inf for none); --frames 0 renders nothing
//             [--raycast CHANNEL ISO DT NSAMPLES REFINE out.hit] where the field of CHANNEL first crosses ISO along the same
//                                            rays (exa_hip_raycast_iso: world space, unit directions, REFINE rounds of
//                                            bisection, NaN for no crossing): one text line `raycast W H channel C iso ISO dt
//                                            DT samples N refine R`, then seven raw little-endian arrays of W x H elements,
//                                            row y = 0 first: t (float32), position (3 float32), value (float32), gradient
//                                            (3 float32), index (int32), side (int32), crossings (uint32); --frames 0 renders
//                                            nothing
//             [--surface MESH C0[,C1,C2,C3] SPACING MAXN out.surf] up to four channels of the field on the triangles of MESH
//                                            (exa_hip_sample_triangles: each triangle cut into n x n parts, n = longest edge /
//                                            SPACING rounded up, at most MAXN, sampled at their centroids), a triangle file as
//                                            --isomesh writes it (all its meshes), or the word `iso`: the mesh of this
//                                            invocation's --isomesh, in its space, integrated where it lies on the device.  Text,
//                                            floats as %.9g and doubles as %.17g: one line `surface triangles T channels C c0 ..
//                                            spacing S maxN N world 0|1`; per triangle one line `subdiv nx ny nz area` (areaNormal
//                                            and its length) followed per channel by `count sum mean integral` (mean = sum / count,
//                                            integral = mean * area, nan for count 0); one line `invalid K` (triangles of subdiv 0,
//                                            left out of the totals); per channel one line `total c covered_area A uncovered_area U
//                                            uncovered_triangles K integral I force fx fy fz` (sums of mean * area and of mean *
//                                            areaNormal, in double in triangle order); with three channels one line `flux F` (the
//                                            sum of mean . areaNormal); with
//             [--surface-world]              a MESH file's vertices are in world space; --frames 0 renders nothing
#include "exa_host.h"

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <iostream>

using namespace exa;

namespace {
using ull = unsigned long long;
[[noreturn]] void fail(const std::string &text) { throw std::runtime_error(text); }

// printf into a string: the line that a file's header and stdout share
__attribute__((format(printf, 1, 2))) std::string format(const char *fmt, ...)
{
  char line[1024];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(line, sizeof(line), fmt, ap);
  va_end(ap);
  return line;
}

// ---- the options: one struct per output, with today's defaults; a file name says that the output is requested
struct PlaneOpts { vec3f origin, du, dv; vec2i size; };      // the lattice of --isolines and --lic: (i,j) at origin + (i + .5) du + (j + .5) dv
struct DerivedOpts {                                         // --derived: resample, isomesh, isolines, regions and basins work on it
  int quantity = -1;                                         // EXA_DERIVED_*, -1: on their channel
  vec3i channels{ 0, 1, 2 };
  bool on() const { return quantity >= 0; }
};
struct LatticeFlags { box3f box; bool haveBox = false, world = false, below = false, faces = false; };   // --regions-*: regions and basins
struct ResampleOpts { std::string name; vec3i dims; int channel = 0; bool haveChannel = false, world = false, haveBox = false; box3f box; float fill = NAN; };
struct IsoMeshOpts { std::string name; float iso = 0.f; vec3i dims; int channel = 0; bool haveChannel = false, world = false, haveBox = false; box3f box; };
struct IsolinesOpts { std::string name; int channel = 0; PlaneOpts plane; std::vector<float> isos; bool world = false; };
struct LicOpts { std::string name; vec3i channels{ 0, 1, 2 }; PlaneOpts plane; float step = 0.5f; int halfLength = 20; uint32_t seed = 0; };
struct FtleOpts { std::string name; vec3i channels{ 0, 1, 2 }, dims{ 1, 1, 1 }; box3f box; float step = 0.5f; int numSteps = 20; bool backward = false; };
struct CriticalOpts { std::string name; vec3i channels{ 0, 1, 2 }, dims{ 2, 2, 2 }; box3f box; int iterations = 8; float tolerance = 0.0009765625f; };
struct RegionsOpts { std::string name; int channel = 0; float iso = 0.f; vec3i dims; };
struct DistanceOpts { std::string name; int channel = 0; float iso = 0.f, maxDistance = INFINITY; vec3i dims; box3f box; bool haveBox = false, isSigned = false, outside = false; };
struct BasinsOpts { std::string name; int channel = 0; float iso = 0.f, minDepth = 0.f; vec3i dims; };
struct ProfileOpts {
  std::string name, axes, values, weight; vec3i dims; box3f box; bool haveBox = false, world = false, log = false;
  // what parseProfile makes of the words: per axis the struct, the edges of --profile-log, `regions` / `basins` for a label axis
  std::vector<ExaHipProfileAxis> axis; std::vector<std::vector<float>> edges; std::vector<std::string> labelsOf;
  std::vector<ExaHipSource> value; ExaHipSource weightSource = {};
};
struct SurfaceOpts { std::string name, mesh; std::vector<int> channels; float spacing = 0.f; int maxN = 0; bool world = false; };   // mesh: a file, or `iso`
struct HistogramOpts { std::string name; int bins = 0, channel = 0; bool haveRange = false, haveBox = false; float range[2] = { 0, 1 }; box3i box; };
struct StreamlinesOpts { std::string seedsName, name; float step = 0.f; int maxSteps = 0; vec3i channels{ 0, 1, 2 }; bool both = false, backward = false, normalize = false; };
struct ProjectOpts { std::string name; int channel = 0, samples = 0; float dt = 0.f; };
struct RaycastOpts { std::string name; int channel = 0, samples = 0, refine = 0; float iso = 0.f, dt = 0.f; };
struct FrameOpts {                                           // what the reference's viewer takes, the devices and the frame loop
  std::string cfgName, outName, xfFile;
  vec2i size{ 600, 400 };                                    // viewer default window
  vec3f vp, vi, vu;                                          // --camera
  float fov = 70.f, dt = 0.5f, xfScale = 1.f, aoLength = 1e20f;
  float isoVals[2] = { 0, 0 }; int isoChans[2] = { 0, 0 }, isoOn[2] = { 0, 0 };
  bool haveRange = false, ao = false, pg = true, skipping = true, gradDVR = true, gradISO = true, info = false, clip = false, stats = false;
  float range[2] = { 0, 1 }; box3f clipBox;
  int frames = 1;
  std::vector<int> devices;
  bool pipeline = false, allowEmptyCells = false;
  std::vector<float> contourPlanes;                          // 4 floats per --contourplane (normal, offset)
  std::vector<int> contourChans;
  std::vector<std::pair<std::string, int>> options;          // --option key=value
};
struct Options {
  FrameOpts frame; DerivedOpts derived; LatticeFlags lattice; ResampleOpts resample; IsoMeshOpts isomesh; IsolinesOpts isolines; LicOpts lic;
  FtleOpts ftle; CriticalOpts critical; RegionsOpts regions; BasinsOpts basins; DistanceOpts distance; ProfileOpts profile; SurfaceOpts surface; HistogramOpts histogram;
  StreamlinesOpts streamlines; ProjectOpts project; RaycastOpts raycast;
};

// ---- the command line: a cursor over argv.  Numbers are read leniently (atof: `1e2` is 100, `x` is 0)
struct Args {
  int argc; char **argv; int i;
  std::string flag;                                          // the word that next() stopped at
  bool next() { if (++i >= argc) return false; flag = argv[i]; return true; }
  // the next word, the error `text` unless `need` more words are there (word(text, 2) makes sure of the word("") after it)
  const char *word(const std::string &text, int need = 1) { if (i + need >= argc) fail(text); return argv[++i]; }
  float number() { return (float)atof(word("missing value after " + flag)); }
  int count() { return (int)number(); }
  int integer() { return (int)std::strtol(word("missing value after " + flag), nullptr, 10); }
  vec3f vec3() { const float x = number(), y = number(), z = number(); return vec3f(x, y, z); }
  vec3i int3() { const int x = count(), y = count(), z = count(); return vec3i(x, y, z); }
  box3f box() { const vec3f lower = vec3(), upper = vec3(); return box3f(lower, upper); }
  PlaneOpts plane() { PlaneOpts p; p.origin = vec3(); p.du = vec3(); p.dv = vec3(); p.size.x = count(); p.size.y = count(); return p; }
  vec3i channels3()                                          // C0,C1,C2 in one word
  {
    vec3i c;
    char tail = 0;
    if (std::sscanf(word("missing channels after " + flag), "%d,%d,%d%c", &c.x, &c.y, &c.z, &tail) != 3)
      fail(flag + " wants three comma-separated channels C0,C1,C2");
    return c;
  }
};

// appends comma-separated numbers within [lo, hi]; the empty list and a comma at the end pass, anything else is the error `text`
template <class T, class Parse>
void appendList(std::vector<T> &out, const char *p, const char *text, Parse parse, double lo = -INFINITY, double hi = INFINITY)
{
  while (*p) {
    char *end = nullptr;
    const auto v = parse(p, &end);
    if (end == p || (*end != ',' && *end != 0) || v < lo || v > hi) fail(text);
    out.push_back((T)v);
    p = *end == ',' ? end + 1 : end;
  }
}
float floatOf(const char *p, char **end) { return std::strtof(p, end); }
long longOf(const char *p, char **end) { return std::strtol(p, end, 10); }

// --derived QUANTITY: a name or a number; EXA_DERIVED_* (the module refuses an unknown number)
int derivedQuantity(const std::string &s)
{
  static const char *const names[EXA_DERIVED_QUANTITIES] = { "speed", "divergence", "vorticity", "vorticity_magnitude", "q", "helicity" };
  for (int q = 0; q < EXA_DERIVED_QUANTITIES; q++)
    if (s == names[q]) return q;
  char *end = nullptr;
  const long q = std::strtol(s.c_str(), &end, 10);
  if (end == s.c_str() || *end || q < 0) fail("--derived wants speed, divergence, vorticity, vorticity_magnitude, q, helicity or a number, not " + s);
  return (int)q;
}

// every parse...Flag(): takes the flag the cursor stands on if it is one of its own; false if it is not
bool parseFrameFlag(Args &a, FrameOpts &o)
{
  const std::string &f = a.flag;
  if (f == "--size" || f == "-win") { o.size.x = a.count(); o.size.y = a.count(); }
  else if (f == "--camera") { o.vp = a.vec3(); o.vi = a.vec3(); o.vu = a.vec3(); }
  else if (f == "--fov") o.fov = a.number();
  else if (f == "--dt") o.dt = a.number();
  else if (f == "--xf") o.xfFile = a.word("missing file after --xf");
  else if (f == "--xf-scale") o.xfScale = a.number();
  else if (f == "--range") { o.range[0] = a.number(); o.range[1] = a.number(); o.haveRange = true; }
  else if (f == "--isovals") { o.isoVals[0] = a.number(); o.isoVals[1] = a.number(); o.isoOn[0] = o.isoOn[1] = 1; }
  else if (f == "--isochans") { o.isoChans[0] = a.count(); o.isoChans[1] = a.count(); }
  else if (f == "--contourplane") { for (int k = 0; k < 4; k++) o.contourPlanes.push_back(a.number()); }   // viewer.cpp:1199-1205
  else if (f == "--contourchan") o.contourChans.push_back(a.count());                                      // viewer.cpp:1206-1207
  else if (f == "--clip-box") { o.clipBox = a.box(); o.clip = true; }
  else if (f == "--ao") o.ao = true;
  else if (f == "--ao-length") o.aoLength = a.number();
  else if (f == "--no-pg") o.pg = false;
  else if (f == "--no-space-skipping") o.skipping = false;
  else if (f == "--gradientShadingDVR") o.gradDVR = a.number() != 0.f;
  else if (f == "--gradientShadingISO") o.gradISO = a.number() != 0.f;
  else if (f == "--frames") o.frames = a.count();
  else if (f == "-o") o.outName = a.word("missing file after -o");
  else if (f == "--info") o.info = true;
  else if (f == "--stats") o.stats = true;
  else if (f == "--gpus") { const int n = a.count(); o.devices.clear(); for (int d = 0; d < n; d++) o.devices.push_back(d); }
  else if (f == "--devices") {                               // stricter than the other lists: not empty, no comma at the end
    const char *text = "--devices wants a comma-separated list of device indices";
    const std::string list = a.word("missing list after --devices");
    o.devices.clear();
    appendList(o.devices, list.c_str(), text, longOf, 0, 1023);
    if (o.devices.empty() || list.back() == ',') fail(text);
  }
  else if (f == "--pipeline") o.pipeline = true;
  else if (f == "--allow-empty-cells") o.allowEmptyCells = true;  // the reference built with -DALLOW_EMPTY_CELLS=1
  else if (f == "--option") {                                // exa_hip_set_option: --option walk=2, --option ao_overlap=0 ...
    const std::string kv = a.word("missing key=value after --option");
    const size_t eq = kv.find('=');
    char *end = nullptr;
    const long v = eq == std::string::npos ? 0 : std::strtol(kv.c_str() + eq + 1, &end, 10);
    if (eq == std::string::npos || eq == 0 || end == kv.c_str() + eq + 1 || *end) fail("--option wants key=integer");
    o.options.emplace_back(kv.substr(0, eq), (int)v);
  }
  else return false;
  return true;
}

// the outputs on a lattice in a box, and what they share
bool parseLatticeOutputFlag(Args &a, Options &o)
{
  const std::string &f = a.flag;
  if (f == "--resample") { o.resample.dims = a.int3(); o.resample.name = a.word("missing file after --resample NX NY NZ"); }
  else if (f == "--resample-box") { o.resample.box = a.box(); o.resample.haveBox = true; }
  else if (f == "--resample-world") o.resample.world = true;
  else if (f == "--resample-channel") { o.resample.channel = a.count(); o.resample.haveChannel = true; }
  else if (f == "--resample-fill") o.resample.fill = a.number();
  else if (f == "--isomesh") {
    o.isomesh.iso = a.number(); o.isomesh.dims = a.int3();
    o.isomesh.name = a.word("missing file after --isomesh ISO NX NY NZ");
  }
  else if (f == "--isomesh-box") { o.isomesh.box = a.box(); o.isomesh.haveBox = true; }
  else if (f == "--isomesh-world") o.isomesh.world = true;
  else if (f == "--isomesh-channel") { o.isomesh.channel = a.count(); o.isomesh.haveChannel = true; }
  else if (f == "--ftle") {
    FtleOpts &t = o.ftle;
    t.channels = a.channels3(); t.box = a.box(); t.dims = a.int3(); t.step = a.number(); t.numSteps = a.count();
    const std::string dir = a.word("missing direction and file after --ftle C0,C1,C2 l u NX NY NZ STEP NUMSTEPS", 2);
    if (dir != "fwd" && dir != "bwd") fail("--ftle wants the direction fwd or bwd");
    t.backward = dir == "bwd";
    t.name = a.word("");
  }
  else if (f == "--critical") {
    CriticalOpts &c = o.critical;
    c.channels = a.channels3(); c.box = a.box(); c.dims = a.int3(); c.iterations = a.count(); c.tolerance = a.number();
    c.name = a.word("missing file after --critical C0,C1,C2 l u NX NY NZ ITERATIONS TOLERANCE");
  }
  else if (f == "--regions") {
    o.regions.channel = a.count(); o.regions.iso = a.number(); o.regions.dims = a.int3();
    o.regions.name = a.word("missing file after --regions CHANNEL ISO NX NY NZ");
  }
  else if (f == "--basins") {
    o.basins.channel = a.count(); o.basins.iso = a.number(); o.basins.minDepth = a.number(); o.basins.dims = a.int3();
    o.basins.name = a.word("missing file after --basins CHANNEL ISO MINDEPTH NX NY NZ");
  }
  else if (f == "--profile") {
    o.profile.axes = a.word("missing axes after --profile");
    o.profile.values = a.word("missing values after --profile AXIS[/AXIS]");
    o.profile.dims = a.int3();
    o.profile.name = a.word("missing file after --profile AXIS[/AXIS] VALUES NX NY NZ");
  }
  else if (f == "--profile-weight") o.profile.weight = a.word("missing source after --profile-weight");
  else if (f == "--profile-box") { o.profile.box = a.box(); o.profile.haveBox = true; }
  else if (f == "--profile-world") o.profile.world = true;
  else if (f == "--profile-log") o.profile.log = true;
  else if (f == "--distance") {
    DistanceOpts &d = o.distance;
    d.channel = a.count(); d.iso = a.number(); d.maxDistance = a.number(); d.dims = a.int3();
    d.name = a.word("missing file after --distance CHANNEL ISO MAXDIST NX NY NZ");
  }
  else if (f == "--distance-box") { o.distance.box = a.box(); o.distance.haveBox = true; }
  else if (f == "--distance-signed") o.distance.isSigned = true;
  else if (f == "--distance-outside") o.distance.outside = true;
  else if (f == "--regions-box") { o.lattice.box = a.box(); o.lattice.haveBox = true; }
  else if (f == "--regions-world") o.lattice.world = true;
  else if (f == "--regions-below") o.lattice.below = true;
  else if (f == "--regions-faces") o.lattice.faces = true;
  else if (f == "--derived") {
    o.derived.quantity = derivedQuantity(a.word("missing quantity after --derived"));
    o.derived.channels = a.int3();
  }
  else return false;
  return true;
}

// the outputs on a plane, on a mesh, on seeds, on the image and on the cells
bool parseOtherOutputFlag(Args &a, Options &o)
{
  const std::string &f = a.flag;
  if (f == "--isolines") {
    o.isolines.channel = a.count(); o.isolines.plane = a.plane();
    const char *levels = a.word("missing levels and file after --isolines CHANNEL o u v NU NV", 2);
    appendList(o.isolines.isos, levels, "--isolines wants a comma-separated list of levels", floatOf);
    o.isolines.name = a.word("");
  }
  else if (f == "--isolines-world") o.isolines.world = true;
  else if (f == "--lic") {
    o.lic.channels = a.channels3(); o.lic.plane = a.plane(); o.lic.step = a.number(); o.lic.halfLength = a.count();
    o.lic.name = a.word("missing file after --lic C0,C1,C2 o u v NU NV STEP HALFLENGTH");
  }
  else if (f == "--lic-seed") o.lic.seed = (uint32_t)std::strtoul(a.word("missing value after --lic-seed"), nullptr, 10);
  else if (f == "--surface") {
    o.surface.mesh = a.word("missing mesh and channels after --surface", 2);
    appendList(o.surface.channels, a.word(""), "--surface: channels are C0[,C1,C2,C3]", longOf);
    o.surface.spacing = a.number(); o.surface.maxN = a.count();
    o.surface.name = a.word("missing file after --surface MESH CHANNELS SPACING MAXN");
  }
  else if (f == "--surface-world") o.surface.world = true;
  else if (f == "--histogram") { o.histogram.bins = a.count(); o.histogram.name = a.word("missing file after --histogram BINS"); }
  else if (f == "--histogram-channel") o.histogram.channel = a.count();
  else if (f == "--histogram-range") { o.histogram.range[0] = a.number(); o.histogram.range[1] = a.number(); o.histogram.haveRange = true; }
  else if (f == "--histogram-box") {                         // integer voxel coordinates: strtol
    for (vec3i *v : { &o.histogram.box.lower, &o.histogram.box.upper }) { v->x = a.integer(); v->y = a.integer(); v->z = a.integer(); }
    o.histogram.haveBox = true;
  }
  else if (f == "--streamlines") {
    o.streamlines.seedsName = a.word("missing seed file after --streamlines");
    o.streamlines.step = a.number(); o.streamlines.maxSteps = a.count();
    o.streamlines.name = a.word("missing file after --streamlines SEEDS.txt STEP MAXSTEPS");
  }
  else if (f == "--streamlines-channels") o.streamlines.channels = a.int3();
  else if (f == "--streamlines-both") o.streamlines.both = true;
  else if (f == "--streamlines-backward") o.streamlines.backward = true;
  else if (f == "--streamlines-normalize") o.streamlines.normalize = true;
  else if (f == "--project") {
    o.project.channel = a.count(); o.project.dt = a.number(); o.project.samples = a.count();
    o.project.name = a.word("missing file after --project CHANNEL DT NSAMPLES");
  }
  else if (f == "--raycast") {
    RaycastOpts &r = o.raycast;
    r.channel = a.count(); r.iso = a.number(); r.dt = a.number(); r.samples = a.count(); r.refine = a.count();
    r.name = a.word("missing file after --raycast CHANNEL ISO DT NSAMPLES REFINE");
  }
  else return false;
  return true;
}

// --profile: a SOURCE word
ExaHipSource profileSource(const std::string &w)
{
  ExaHipSource s = {};
  char tail = 0;
  const size_t colon = w.find(':');
  if (w == "x" || w == "y" || w == "z") { s.kind = EXA_SOURCE_COORDINATE; s.channels[0] = w[0] - 'x'; }
  else if (w.size() > 1 && w[0] == 'c' && std::sscanf(w.c_str() + 1, "%d%c", &s.channels[0], &tail) == 1) s.kind = EXA_SOURCE_CHANNEL;
  else if (w.compare(0, 2, "r:") == 0 && std::sscanf(w.c_str() + 2, "%f,%f,%f%c", &s.centre[0], &s.centre[1], &s.centre[2], &tail) == 3) s.kind = EXA_SOURCE_RADIUS;
  else if (colon != std::string::npos && colon >= 1
           && std::sscanf(w.c_str() + colon + 1, "%d,%d,%d%c", &s.channels[0], &s.channels[1], &s.channels[2], &tail) == 3) {
    s.kind = EXA_SOURCE_DERIVED;
    s.quantity = derivedQuantity(w.substr(0, colon));
  }
  else fail("--profile wants a source cN, QUANTITY:C0,C1,C2, r:x,y,z, x, y or z, not " + w);
  return s;
}

std::vector<std::string> splitWords(const std::string &s, char at)
{
  std::vector<std::string> out(1);
  for (char c : s) { if (c == at) out.emplace_back(); else out.back() += c; }
  return out;
}

// the words of --profile and --profile-weight, once every flag is read: the sources, the axes with the edges of --profile-log,
// and whether the --regions / --basins that a label axis names is there on the same lattice
void parseProfile(Options &all)
{
  ProfileOpts &o = all.profile;
  const std::vector<std::string> axisWords = splitWords(o.axes, '/');
  if (axisWords.size() > 2) fail("--profile wants one or two axes AXIS[/AXIS]");
  o.edges.resize(axisWords.size());
  for (size_t k = 0; k < axisWords.size(); k++) {
    const std::string &w = axisWords[k];
    ExaHipProfileAxis ax = {};
    o.labelsOf.push_back(w == "regions" || w == "basins" ? w : "");
    if (!o.labelsOf[k].empty()) {
      if (k) fail("--profile takes " + w + " as its first axis only");
      const bool regions = w == "regions";
      const vec3i d = regions ? all.regions.dims : all.basins.dims;
      const LatticeFlags &lf = all.lattice;
      if ((regions ? all.regions.name : all.basins.name).empty() || lf.world != o.world || d.x != o.dims.x || d.y != o.dims.y || d.z != o.dims.z
          || lf.haveBox != o.haveBox || (o.haveBox && std::memcmp(&lf.box, &o.box, sizeof(o.box)) != 0))
        fail("--profile " + w + " needs --" + w + " on the same lattice in the same invocation");
    } else {
      const size_t at = w.find('@');
      char tail = 0;
      if (at == std::string::npos || std::sscanf(w.c_str() + at + 1, "%f:%f:%d%c", &ax.lo, &ax.hi, &ax.numBins, &tail) != 3)
        fail("--profile wants an axis SOURCE@LO:HI:BINS, regions or basins, not " + w);
      ax.source = profileSource(w.substr(0, at));
      if (o.log) {
        const char *text = "--profile-log wants edges LO * (HI / LO)^(b / BINS) that ascend strictly (0 < LO < HI, BINS >= 1 and not too many)";
        if (!(ax.lo > 0.f && ax.hi > ax.lo && ax.numBins >= 1 && ax.numBins <= EXA_PROFILE_MAX_BINS)) fail(text);
        for (int b = 0; b <= ax.numBins; b++) {
          o.edges[k].push_back(float(double(ax.lo) * std::pow(double(ax.hi) / double(ax.lo), double(b) / double(ax.numBins))));
          if (b && !(o.edges[k][b] > o.edges[k][b - 1])) fail(text);
        }
      }
    }
    o.axis.push_back(ax);
  }
  if (o.values != "none")
    for (const std::string &w : splitWords(o.values, '+')) o.value.push_back(profileSource(w));
  if (o.value.size() > EXA_PROFILE_MAX_VALUES) fail("--profile wants at most 4 values");
  if (!o.weight.empty()) o.weightSource = profileSource(o.weight);
}

Options parseOptions(int argc, char **argv)
{
  Options o;
  Args a{ argc, argv, 0, "" };
  while (a.next()) {
    if (parseFrameFlag(a, o.frame) || parseLatticeOutputFlag(a, o) || parseOtherOutputFlag(a, o)) continue;
    if (a.flag[0] != '-') o.frame.cfgName = a.flag;          // a word that is no flag: the config
    else fail("unknown flag " + a.flag);
  }
  if (o.frame.cfgName.empty()) fail("usage: exaRender cfg.exa [flags]");
  if (o.derived.on() && (o.resample.haveChannel || o.isomesh.haveChannel))
    fail("--derived takes its three channels itself: --resample-channel / --isomesh-channel do not go with it");
  if (!o.profile.name.empty()) parseProfile(o);
  return o;
}

// ---- what the outputs share: files, the words for the field they work on, the default box
FILE *openFile(const std::string &name, const char *mode)
{
  FILE *f = std::fopen(name.c_str(), mode);
  if (!f) fail("cannot write " + name);
  return f;
}
void closeFile(FILE *f, const std::string &name) { if (std::fclose(f)) fail("cannot write " + name); }

// a file of one header line (none if empty) and raw arrays
struct Array { const void *data; size_t elementSize, count; };
void writeRaw(const std::string &name, const std::string &header, std::initializer_list<Array> arrays)
{
  FILE *f = openFile(name, "wb");
  bool ok = std::fputs(header.c_str(), f) >= 0;
  for (const Array &a : arrays) ok = ok && std::fwrite(a.data, a.elementSize, a.count, f) == a.count;
  if (std::fclose(f) || !ok) fail("cannot write " + name);
}

std::string fieldWords(const DerivedOpts &dv, int channel)
{
  return dv.on() ? format("derived %d channels %d %d %d ", dv.quantity, dv.channels.x, dv.channels.y, dv.channels.z)
                 : format("channel %d ", channel);
}

// the box of an output that was given none: everything, in the space it works in
box3f boxOr(bool have, const box3f &box, bool world, const Renderer &r) { return have ? box : (world ? r.worldSpaceBounds : r.voxelSpaceBounds); }

std::string latticeWords(const char *what, vec3i dims, const box3f &box)
{
  return format("%s %d %d %d box %.9g %.9g %.9g %.9g %.9g %.9g ", what, dims.x, dims.y, dims.z, box.lower.x, box.lower.y, box.lower.z,
                box.upper.x, box.upper.y, box.upper.z);
}

// ---- the outputs, one function each: the call, the file, the line on stdout.  The next one gets a struct above, its flags in
// a parse...Flag(), a function here and a line in writeOutputs below.
void writeResample(const ResampleOpts &o, const DerivedOpts &dv, Renderer &r)
{
  const box3f box = boxOr(o.haveBox, o.box, o.world, r);
  if (o.dims.x < 1 || o.dims.y < 1 || o.dims.z < 1) fail("--resample wants NX NY NZ >= 1");
  const size_t comps = dv.quantity == EXA_DERIVED_VORTICITY ? 3 : 1;
  std::vector<float> grid(size_t(o.dims.x) * size_t(o.dims.y) * size_t(o.dims.z) * comps);
  // sampled with a NaN fill to count the points outside every region (a reconstructed value is never NaN for a field
  // without NaNs), then the requested fill written in their place
  if (dv.on()) r.resampleDerived(box, o.dims, dv.channels, dv.quantity, grid.data(), o.world, NAN);
  else r.resample(box, o.dims, o.channel, grid.data(), o.world, NAN);
  size_t invalid = 0;                                        // floats: `comps` per lattice point
  for (float &v : grid)
    if (std::isnan(v)) { v = o.fill; invalid++; }
  writeRaw(o.name, "", { { grid.data(), sizeof(float), grid.size() } });
  std::printf("%s%s", latticeWords("resample", o.dims, box).c_str(), fieldWords(dv, o.channel).c_str());
  if (dv.on()) std::printf("components %zu ", comps);
  std::printf("invalid %zu\n", invalid);
}

// what --surface iso needs of this invocation's --isomesh: the mesh that the module kept
struct KeptIsoMesh { bool present; bool world; size_t triangles; };

KeptIsoMesh writeIsoMesh(const IsoMeshOpts &o, const DerivedOpts &dv, bool keep, Renderer &r)
{
  const box3f box = boxOr(o.haveBox, o.box, o.world, r);
  TriangleMesh::SP mesh = dv.on() ? r.extractIsoSurfaceDerived(box, o.dims, dv.channels, dv.quantity, o.iso, o.world, keep)
                                  : r.extractIsoSurface(box, o.dims, o.channel, o.iso, o.world, nullptr, keep);
  TriangleMesh::save(o.name, { mesh });
  std::printf("%s%siso %.9g vertices %zu triangles %zu\n", latticeWords("isomesh", o.dims, box).c_str(), fieldWords(dv, o.channel).c_str(),
              o.iso, mesh->vertex.size(), mesh->index.size());
  return { true, o.world, mesh->index.size() };
}

void writeIsolines(const IsolinesOpts &o, const DerivedOpts &dv, Renderer &r)
{
  const PlaneOpts &p = o.plane;
  const Renderer::Isolines L = dv.on() ? r.isolinesDerived(p.origin, p.du, p.dv, p.size, o.isos, dv.channels, dv.quantity, o.world)
                                       : r.isolines(p.origin, p.du, p.dv, p.size, o.isos, o.channel, o.world);
  const size_t n = o.isos.size(), nv = L.vertex.size(), ns = L.segment.size() / 2;
  writeRaw(o.name, format("isolines %d %d levels %zu vertices %zu segments %zu\n", p.size.x, p.size.y, n, nv, ns),
           { { o.isos.data(), 4, n }, { L.vertexOffsets.data(), 8, n + 1 }, { L.segmentOffsets.data(), 8, n + 1 },
             { L.vertex.data(), 12, nv }, { L.uv.data(), 8, nv }, { L.segment.data(), 8, ns } });
  std::printf("isolines %d %d %sworld %d levels %zu vertices %zu segments %zu\n", p.size.x, p.size.y, fieldWords(dv, o.channel).c_str(),
              o.world ? 1 : 0, n, nv, ns);
}

void writeLic(const LicOpts &o, Renderer &r)
{
  const PlaneOpts &p = o.plane;
  const Renderer::Lic L = r.lic(p.origin, p.du, p.dv, p.size, o.channels, o.step, o.halfLength, nullptr, o.seed);
  const std::string head = format("lic %d %d channels %d %d %d step %.9g halfLength %d seed %u", p.size.x, p.size.y, o.channels.x,
                                  o.channels.y, o.channels.z, o.step, o.halfLength, o.seed);
  writeRaw(o.name, head + "\n", { { L.lic.data(), 4, L.lic.size() } });
  size_t covered = 0;
  ull samples = 0;
  for (uint32_t c : L.count) { covered += c > 0; samples += c; }
  std::printf("%s pixels_covered %zu samples %llu\n", head.c_str(), covered, samples);
}

void writeFtle(const FtleOpts &o, Renderer &r)
{
  const Renderer::Flowmap M = r.flowmap(o.box.lower, o.box.upper, o.dims, o.channels, o.step, o.numSteps, o.backward);
  const std::string head = format("ftle %d %d %d channels %d %d %d step %.9g numSteps %d direction %s", o.dims.x, o.dims.y, o.dims.z,
                                  o.channels.x, o.channels.y, o.channels.z, o.step, o.numSteps, o.backward ? "bwd" : "fwd");
  const size_t n = M.stretch.size();
  writeRaw(o.name, head + "\n",
           { { M.end.data(), 12, n }, { M.steps.data(), 4, n }, { M.reason.data(), 4, n }, { M.stretch.data(), 4, n }, { M.ftle.data(), 4, n } });
  size_t valid = 0;
  for (float v : M.ftle) valid += !std::isnan(v);
  std::printf("%s points_with_ftle %zu\n", head.c_str(), valid);
}

void writeCritical(const CriticalOpts &o, Renderer &r)
{
  const Renderer::CriticalPoints P = r.criticalPoints(o.box, o.dims, o.channels, o.iterations, o.tolerance);
  const ExaHipCriticalStats &st = P.stats;
  const std::string head = latticeWords("critical", o.dims, o.box)
                         + format("channels %d %d %d iterations %d tolerance %.9g cells %llu invalidCells %llu candidates %llu found %llu "
                                  "nonFinite %llu leftCell %llu notConverged %llu", o.channels.x, o.channels.y, o.channels.z, o.iterations,
                                  o.tolerance, ull(st.cells), ull(st.invalidCells), ull(st.candidates), ull(st.found), ull(st.nonFinite),
                                  ull(st.leftCell), ull(st.notConverged));
  writeRaw(o.name, head + "\n", { { P.points.data(), sizeof(ExaHipCriticalPoint), P.points.size() } });
  // the found points by n+ (sink, the two saddles, source) and, of each, the spiralling ones
  size_t kind[4] = { 0, 0, 0, 0 }, spiral[4] = { 0, 0, 0, 0 }, degenerate = 0;
  for (const ExaHipCriticalPoint &p : P.points) {
    kind[p.type & 3]++;
    spiral[p.type & 3] += (p.type & EXA_CRITICAL_SPIRAL) ? 1 : 0;
    degenerate += (p.type & EXA_CRITICAL_DEGENERATE) ? 1 : 0;
  }
  std::printf("%s sinks %zu spiral %zu saddles1 %zu spiral %zu saddles2 %zu spiral %zu sources %zu spiral %zu degenerate %zu\n", head.c_str(),
              kind[0], spiral[0], kind[1], spiral[1], kind[2], spiral[2], kind[3], spiral[3], degenerate);
}

// the labels of this invocation's --regions or --basins for --profile regions / basins, kept the way --surface iso keeps the mesh
struct KeptLabels { bool present = false, world = false; vec3i dims; box3f box; int32_t count = 0; std::vector<int32_t> labels; };

template <class Labelling>
void keepLabels(KeptLabels *keep, const Labelling &L, size_t count, vec3i dims, const box3f &box, bool world)
{
  if (!keep) return;
  keep->present = true; keep->world = world; keep->dims = dims; keep->box = box; keep->count = int32_t(count); keep->labels = L.labels;
}

void writeRegions(const RegionsOpts &o, const LatticeFlags &lf, const DerivedOpts &dv, KeptLabels *keep, Renderer &r)
{
  const box3f box = boxOr(lf.haveBox, lf.box, lf.world, r);
  const Renderer::Regions R = dv.on() ? r.regionsDerived(box, o.dims, dv.channels, dv.quantity, o.iso, lf.world, lf.below, lf.faces)
                                      : r.regions(box, o.dims, o.channel, o.iso, lf.world, lf.below, lf.faces);
  const std::string counts = format("count %zu inside %llu exponent %d\n", R.regions.size(), ull(R.numInside), R.sumExponent);
  writeRaw(o.name, format("regions %d %d %d ", o.dims.x, o.dims.y, o.dims.z) + counts,
           { { R.regions.data(), sizeof(ExaHipRegion), R.regions.size() }, { R.labels.data(), 4, R.labels.size() } });
  std::printf("regions %d %d %d %siso %.9g world %d below %d faces %d %s", o.dims.x, o.dims.y, o.dims.z, fieldWords(dv, o.channel).c_str(),
              o.iso, lf.world ? 1 : 0, lf.below ? 1 : 0, lf.faces ? 1 : 0, counts.c_str());
  keepLabels(keep, R, R.regions.size(), o.dims, box, lf.world);
}

void writeBasins(const BasinsOpts &o, const LatticeFlags &lf, const DerivedOpts &dv, KeptLabels *keep, Renderer &r)
{
  const box3f box = boxOr(lf.haveBox, lf.box, lf.world, r);
  const Renderer::Basins B = dv.on() ? r.basinsDerived(box, o.dims, dv.channels, dv.quantity, o.iso, o.minDepth, lf.world, lf.below, lf.faces)
                                     : r.basins(box, o.dims, o.channel, o.iso, o.minDepth, lf.world, lf.below, lf.faces);
  const std::string counts = format("count %zu raw %llu rounds %d inside %llu exponent %d\n", B.basins.size(), ull(B.numRaw), B.rounds,
                                    ull(B.numInside), B.sumExponent);
  writeRaw(o.name, format("basins %d %d %d ", o.dims.x, o.dims.y, o.dims.z) + counts,
           { { B.basins.data(), sizeof(ExaHipBasin), B.basins.size() }, { B.labels.data(), 4, B.labels.size() } });
  std::printf("basins %d %d %d %siso %.9g minDepth %.9g world %d below %d faces %d %s", o.dims.x, o.dims.y, o.dims.z,
              fieldWords(dv, o.channel).c_str(), o.iso, o.minDepth, lf.world ? 1 : 0, lf.below ? 1 : 0, lf.faces ? 1 : 0, counts.c_str());
  keepLabels(keep, B, B.basins.size(), o.dims, box, lf.world);
}

void writeDistance(const DistanceOpts &o, const DerivedOpts &dv, Renderer &r)
{
  const box3f box = boxOr(o.haveBox, o.box, false, r);
  const int flags = (o.isSigned ? EXA_DISTANCE_SIGNED : 0) | (o.outside ? EXA_DISTANCE_TO_OUTSIDE : 0);
  const Renderer::Distance D = dv.on() ? r.distanceDerived(box, o.dims, dv.channels, dv.quantity, o.iso, o.maxDistance, flags, true)
                                       : r.distance(box, o.dims, o.channel, o.iso, o.maxDistance, flags, true);
  const std::string counts = format("points %llu inside %llu reached %llu maxDistance %.9g\n", ull(D.stats.points), ull(D.stats.inside),
                                    ull(D.stats.reached), D.stats.maxDistance);
  writeRaw(o.name, format("distance %d %d %d ", o.dims.x, o.dims.y, o.dims.z) + counts,
           { { D.dist.data(), 4, D.dist.size() }, { D.nearest.data(), 4, D.nearest.size() } });
  std::printf("distance %d %d %d %siso %.9g maxDistance %.9g signed %d outside %d %s", o.dims.x, o.dims.y, o.dims.z,
              fieldWords(dv, o.channel).c_str(), o.iso, o.maxDistance, o.isSigned ? 1 : 0, o.outside ? 1 : 0, counts.c_str());
}

void writeProfile(const ProfileOpts &o, const KeptLabels &regions, const KeptLabels &basins, Renderer &r)
{
  const box3f box = boxOr(o.haveBox, o.box, o.world, r);
  std::vector<ExaHipProfileAxis> axes = o.axis;
  for (size_t k = 0; k < axes.size(); k++) {
    if (!o.edges[k].empty()) axes[k].edges = o.edges[k].data();
    if (o.labelsOf[k].empty()) continue;
    const KeptLabels &kept = o.labelsOf[k] == "regions" ? regions : basins;       // on the same lattice: parseProfile has seen to it
    axes[k].numBins = kept.count;
    axes[k].labels = kept.labels.data();
  }
  const std::vector<ExaHipSource> &values = o.value;
  const ExaHipSource &weight = o.weightSource;
  const Renderer::Profile P = r.profile(box, o.dims, axes, values, o.weight.empty() ? nullptr : &weight, o.world);
  const ExaHipProfileStats &st = P.stats;
  const std::string head = format("profile %d %d %d bins %d %d values %zu weighted %d points %llu outside %llu invalid %llu under %llu %llu "
                                  "over %llu %llu binned %llu weightExponent %d valueExponents %d %d %d %d", o.dims.x, o.dims.y, o.dims.z,
                                  axes[0].numBins, axes.size() > 1 ? axes[1].numBins : 1, values.size(), o.weight.empty() ? 0 : 1,
                                  ull(st.points), ull(st.outside), ull(st.invalid), ull(st.under[0]), ull(st.under[1]), ull(st.over[0]),
                                  ull(st.over[1]), ull(st.binned), st.weightExponent, st.valueExponent[0], st.valueExponent[1],
                                  st.valueExponent[2], st.valueExponent[3]);
  writeRaw(o.name, head + "\n", { { P.count.data(), 8, P.count.size() }, { P.sumWeight.data(), 8, P.sumWeight.size() },
                                  { P.sums.data(), 8, P.sums.size() }, { P.mins.data(), 4, P.mins.size() }, { P.maxs.data(), 4, P.maxs.size() } });
  std::printf("%s world %d log %d lds %d\n", head.c_str(), o.world ? 1 : 0, o.log ? 1 : 0, st.ldsTable);
}

void writeSurface(const SurfaceOpts &o, const KeptIsoMesh &iso, Renderer &r)
{
  const bool fromIso = o.mesh == "iso";
  if (fromIso && !iso.present) fail("--surface iso needs --isomesh in the same invocation");
  Renderer::SurfaceSamples S;
  const bool world = fromIso ? iso.world : o.world;
  if (fromIso) S = r.sampleIsoSurface(iso.triangles, o.channels.data(), (int)o.channels.size(), o.spacing, o.maxN, world);
  else {
    TriangleMesh all;                                        // the file's meshes as one
    for (const TriangleMesh::SP &m : TriangleMesh::load(o.mesh)) {
      const int base = (int)all.vertex.size();
      all.vertex.insert(all.vertex.end(), m->vertex.begin(), m->vertex.end());
      for (const vec3i &t : m->index) all.index.push_back(vec3i(t.x + base, t.y + base, t.z + base));
    }
    S = r.sampleTriangles(all, o.channels.data(), (int)o.channels.size(), o.spacing, o.maxN, world);
  }
  const Renderer::SurfaceIntegrals I = Renderer::surfaceIntegrals(S);
  const size_t nt = S.subdiv.size(), nc = o.channels.size();
  FILE *f = openFile(o.name, "wb");
  std::fprintf(f, "surface triangles %zu channels %zu", nt, nc);
  for (int c : o.channels) std::fprintf(f, " %d", c);
  std::fprintf(f, " spacing %.9g maxN %d world %d\n", o.spacing, o.maxN, world ? 1 : 0);
  for (size_t t = 0; t < nt; t++) {
    std::fprintf(f, "%d %.9g %.9g %.9g %.17g", S.subdiv[t], S.areaNormal[t].x, S.areaNormal[t].y, S.areaNormal[t].z, I.area[t]);
    for (size_t c = 0; c < nc; c++)
      std::fprintf(f, " %u %.17g %.17g %.17g", S.count[t * nc + c], S.sum[t * nc + c], I.mean[t * nc + c], I.integral[t * nc + c]);
    std::fprintf(f, "\n");
  }
  std::fprintf(f, "invalid %llu\n", ull(I.invalidTriangles));
  for (size_t c = 0; c < nc; c++)
    std::fprintf(f, "total %d covered_area %.17g uncovered_area %.17g uncovered_triangles %llu integral %.17g force %.17g %.17g %.17g\n",
                 o.channels[c], I.coveredArea[c], I.uncoveredArea[c], ull(I.uncoveredTriangles[c]), I.totalIntegral[c], I.force[3 * c],
                 I.force[3 * c + 1], I.force[3 * c + 2]);
  if (nc == 3) std::fprintf(f, "flux %.17g\n", I.flux);
  closeFile(f, o.name);
  std::printf("surface triangles %zu channels %zu spacing %.9g maxN %d invalid %llu\n", nt, nc, o.spacing, o.maxN, ull(I.invalidTriangles));
}

void writeHistogram(const HistogramOpts &o, Renderer &r)
{
  if (o.bins < 1) fail("--histogram wants BINS >= 1");
  const box3i *box = o.haveBox ? &o.box : nullptr;
  interval<float> range(o.range[0], o.range[1]);
  if (!o.haveRange) {
    const ExaHipFieldStats s = r.fieldStats(o.channel, box);
    if (!(s.min < s.max)) fail("--histogram: the field is constant (or has no value) there: give --histogram-range lo hi");
    range = interval<float>(s.min, s.max);
  }
  std::vector<uint64_t> cells, volume;
  ExaHipFieldStats st;
  r.computeHistogram(o.channel, range, o.bins, cells, &volume, &st, box);
  FILE *f = openFile(o.name, "w");
  for (size_t b = 0; b < cells.size(); b++) std::fprintf(f, "%llu %llu\n", ull(cells[b]), ull(volume[b]));
  closeFile(f, o.name);
  std::printf("histogram channel %d bins %d range %.9g %.9g slots %llu empty %llu nan %llu under %llu over %llu binned %llu\n", o.channel,
              o.bins, range.lower, range.upper, ull(st.slots), ull(st.empty), ull(st.nan), ull(st.under), ull(st.over), ull(st.binned));
}

void writeStreamlines(const StreamlinesOpts &o, Renderer &r)
{
  std::vector<vec3f> seeds;
  FILE *f = std::fopen(o.seedsName.c_str(), "r");
  if (!f) fail("cannot read " + o.seedsName);
  char word[3][64];
  int got;
  while ((got = std::fscanf(f, "%63s %63s %63s", word[0], word[1], word[2])) == 3)     // strtof: nan and inf are seeds too
    seeds.push_back(vec3f(std::strtof(word[0], nullptr), std::strtof(word[1], nullptr), std::strtof(word[2], nullptr)));
  std::fclose(f);
  if (got != EOF) fail(o.seedsName + ": a seed is three numbers `x y z`");
  const Renderer::Streamlines L = r.streamlines(seeds.data(), seeds.size(), o.channels, o.step, o.maxSteps, o.both || !o.backward,
                                                o.both || o.backward, o.normalize);
  f = openFile(o.name, "w");
  for (size_t i = 0; i < seeds.size(); i++) {
    std::fprintf(f, "%u %d %d %llu", L.seedVertex[i], L.reason[2 * i], L.reason[2 * i + 1], ull(L.offset[i + 1] - L.offset[i]));
    for (uint64_t v = L.offset[i]; v < L.offset[i + 1]; v++) std::fprintf(f, " %.9g %.9g %.9g", L.vertex[v].x, L.vertex[v].y, L.vertex[v].z);
    std::fprintf(f, "\n");
  }
  closeFile(f, o.name);
  std::printf("streamlines seeds %zu channels %d %d %d step %.9g maxSteps %d vertices %zu\n", seeds.size(), o.channels.x, o.channels.y,
              o.channels.z, o.step, o.maxSteps, L.vertex.size());
}

void writeProject(const ProjectOpts &o, vec2i size, Renderer &r)
{
  const Renderer::Projection P = r.project(r.cameraRays(size, 0.f, o.dt, o.samples), o.channel, true, true);
  std::vector<float> integral(P.sum.size());
  size_t hit = 0;
  for (size_t k = 0; k < integral.size(); k++) { integral[k] = float(P.sum[k] * double(o.dt)); hit += P.count[k] != 0; }
  const std::string head = format("project %d %d channel %d dt %.9g samples %d", size.x, size.y, o.channel, o.dt, o.samples);
  const size_t n = integral.size();
  writeRaw(o.name, head + "\n", { { integral.data(), 4, n }, { P.count.data(), 4, n }, { P.max.data(), 4, n }, { P.min.data(), 4, n } });
  std::printf("%s pixels_hit %zu\n", head.c_str(), hit);
}

void writeRaycast(const RaycastOpts &o, vec2i size, Renderer &r)
{
  const Renderer::IsoHits R = r.raycastIso(r.cameraRays(size, 0.f, o.dt, o.samples), o.channel, o.iso, o.refine, true, true);
  const std::string head = format("raycast %d %d channel %d iso %.9g dt %.9g samples %d refine %d", size.x, size.y, o.channel, o.iso, o.dt,
                                  o.samples, o.refine);
  const size_t n = R.t.size();
  writeRaw(o.name, head + "\n",
           { { R.t.data(), 4, n }, { R.position.data(), 12, n }, { R.value.data(), 4, n }, { R.gradient.data(), 12, n },
             { R.index.data(), 4, n }, { R.side.data(), 4, n }, { R.crossings.data(), 4, n } });
  size_t hit = 0;
  for (int32_t k : R.index) hit += k >= 0;
  std::printf("%s pixels_hit %zu\n", head.c_str(), hit);
}

// the requested outputs, in the order of their lines on stdout; whether there was any
bool writeOutputs(const Options &o, Renderer &r)
{
  bool any = false;
  auto wanted = [&any](const std::string &name) { any |= !name.empty(); return !name.empty(); };
  KeptIsoMesh isoMesh{ false, false, 0 };
  if (wanted(o.resample.name)) writeResample(o.resample, o.derived, r);
  if (wanted(o.isomesh.name)) isoMesh = writeIsoMesh(o.isomesh, o.derived, o.surface.mesh == "iso", r);   // --surface iso reads the module's copy
  if (wanted(o.isolines.name)) writeIsolines(o.isolines, o.derived, r);
  if (wanted(o.lic.name)) writeLic(o.lic, r);
  if (wanted(o.ftle.name)) writeFtle(o.ftle, r);
  if (wanted(o.critical.name)) writeCritical(o.critical, r);
  const bool profile = !o.profile.name.empty();
  KeptLabels regionLabels, basinLabels;                      // --profile regions / basins reads them
  if (wanted(o.regions.name)) writeRegions(o.regions, o.lattice, o.derived, profile ? &regionLabels : nullptr, r);
  if (wanted(o.basins.name)) writeBasins(o.basins, o.lattice, o.derived, profile ? &basinLabels : nullptr, r);
  if (wanted(o.profile.name)) writeProfile(o.profile, regionLabels, basinLabels, r);
  if (wanted(o.distance.name)) writeDistance(o.distance, o.derived, r);
  if (wanted(o.surface.name)) writeSurface(o.surface, isoMesh, r);
  if (wanted(o.histogram.name)) writeHistogram(o.histogram, r);
  if (wanted(o.streamlines.name)) writeStreamlines(o.streamlines, r);
  if (wanted(o.project.name)) writeProject(o.project, o.frame.size, r);
  if (wanted(o.raycast.name)) writeRaycast(o.raycast, o.frame.size, r);
  return any;
}

// ---- the renderer and its frames
// glutViewer/Camera.cpp:94-120 + glutViewer/OWLViewer.cpp:69-109 + exa/viewer.cpp:226-238
void setupCamera(Renderer &r, vec3f origin, vec3f interest, vec3f up, float fovy, vec2i size)
{
  vec3f vz = (interest == origin) ? vec3f(0, 0, 1) : -normalize(interest - origin);
  vec3f vx = cross(up, vz);
  vx = dot(vx, vx) < 1e-8f ? vec3f(0, 1, 0) : normalize(vx);
  vec3f vy = normalize(cross(vz, vx));
  const float focal = length(interest - origin);
  if (std::fabs(dot(vz, up)) >= 1e-6f) { vx = normalize(cross(up, vz)); vy = normalize(cross(vz, vx)); }
  auto eps = [](vec3f v) { return std::fmax(std::fmax(std::fabs(v.x), std::fabs(v.y)), std::fabs(v.z)) * float(1. / (1 << 21)); };
  const float fd = std::fmax(std::fmax(eps(origin), eps(vx)), focal);
  const float screen_height = 2.f * tanf(fovy / 2.f * (float)M_PI / 180.f) * fd;
  const vec3f vertical = screen_height * vy;
  const vec3f horizontal = (screen_height * (size.x / float(size.y))) * vx;
  const vec3f lower_left = (-fd) * vz - 0.5f * vertical - 0.5f * horizontal;
  const vec3f du = horizontal / float(size.x), dv = vertical / float(size.y);
  std::printf("camera %.9g %.9g %.9g  %.9g %.9g %.9g  %.9g %.9g %.9g  %.9g %.9g %.9g\n", origin.x, origin.y, origin.z,
              lower_left.x, lower_left.y, lower_left.z, du.x, du.y, du.z, dv.x, dv.y, dv.z);
  r.updateCamera(origin, lower_left, du, dv);
}

// the state of a new renderer as the viewer sets it before its first frame
void setupRenderer(Renderer &renderer, const FrameOpts &o, const Config &config, const box3f &bounds, std::vector<uint32_t> &fb)
{
  for (const auto &kv : o.options) renderer.setOption(kv.first, kv.second);
  if (o.devices.size() > 1) std::printf("devices %zu\n", o.devices.size());
  renderer.setVoxelSpaceTransform(config.bricks.voxelSpaceTransform);
  renderer.resizeFrameBuffer(fb.data(), o.size);
  if (o.vu != vec3f(0.f)) setupCamera(renderer, o.vp, o.vi, o.vu, o.fov, o.size);
  else setupCamera(renderer, bounds.center() + vec3f(-.3f, .7f, 1.f) * bounds.span(), bounds.center(), vec3f(0, 1, 0), 70.f, o.size);

  // default transfer function: alpha ramp, grey ramp colour (the PNG colormaps are UI assets)
  std::vector<float> alpha(NUM_XF_VALUES);
  std::vector<vec3f> color(NUM_XF_VALUES);
  for (int i = 0; i < NUM_XF_VALUES; i++) { alpha[i] = i / float(NUM_XF_VALUES - 1); color[i] = vec3f(alpha[i]); }
  if (!o.xfFile.empty()) {                                   // 128 raw floats (viewer.cpp:139-145,1147-1152)
    FILE *f = std::fopen(o.xfFile.c_str(), "rb");
    if (!f || std::fread(alpha.data(), sizeof(float), NUM_XF_VALUES, f) != (size_t)NUM_XF_VALUES) fail("cannot read " + o.xfFile);
    std::fclose(f);
  }
  for (size_t c = 0; c < config.scalarFields.size(); c++) {  // viewer.cpp:567-575
    interval<float> dom = config.scalarFields[c]->valueRange;
    if (o.haveRange) dom = interval<float>(o.range[0], o.range[1]);
    renderer.updateXF((int)c, alpha.data(), color, dom, o.xfScale);
  }
  renderer.updateIsoValues(o.isoVals, o.isoChans, o.isoOn);
  if (!o.contourPlanes.empty()) {
    // the viewer's contour panel set-up (viewer.cpp:673-690): planes given on the command line are enabled, the
    // others keep their defaults (axis i % 3, offset .5, off); the channels apply when more than one was given
    vec3f n[MAX_CONTOUR_PLANES]; float off[MAX_CONTOUR_PLANES]; int ch[MAX_CONTOUR_PLANES], en[MAX_CONTOUR_PLANES];
    if (o.contourPlanes.size() / 4 > (size_t)MAX_CONTOUR_PLANES) fail("too many contour planes");
    for (int i = 0; i < MAX_CONTOUR_PLANES; i++) {
      if (o.contourPlanes.size() / 4 > (size_t)i) {
        n[i] = vec3f(o.contourPlanes[4 * i], o.contourPlanes[4 * i + 1], o.contourPlanes[4 * i + 2]);
        off[i] = o.contourPlanes[4 * i + 3]; en[i] = 1;
      } else {
        n[i] = vec3f(i % 3 == 0 ? 1.f : 0.f, i % 3 == 1 ? 1.f : 0.f, i % 3 == 2 ? 1.f : 0.f);
        off[i] = .5f; en[i] = 0;
      }
      ch[i] = (o.contourChans.size() > 1 && (size_t)i < o.contourChans.size()) ? o.contourChans[i] : 0;
    }
    renderer.updateContourPlanes(n, off, ch, en);
  }
  renderer.setSpaceSkipping(o.skipping);
  renderer.setGradientShadingDVR(o.gradDVR);
  renderer.setGradientShadingISO(o.gradISO);
  renderer.frameState.ao.enabled = o.ao;                     // viewer.cpp:944-959
  renderer.frameState.ao.length = o.aoLength;
  renderer.frameState.clipBox.enabled = o.clip;
  if (o.clip) {
    const box3f wb = renderer.worldSpaceBounds;
    renderer.frameState.clipBox.coords.lower = wb.lower + o.clipBox.lower * wb.span();
    renderer.frameState.clipBox.coords.upper = wb.lower + o.clipBox.upper * wb.span();
  }
}

// --pipeline: two device frames + two pinned host frames, the march of frame k+1 runs while frame k travels to the host.
// Leaves the last frame in fb and returns the kernel time of all frames
double renderPipelined(Renderer &renderer, const FrameOpts &o, std::vector<uint32_t> &fb)
{
  auto ok = [](hipError_t e, const char *what) { if (e != hipSuccess) fail(std::string(what) + ": " + hipGetErrorString(e)); };
  ok(hipSetDevice(o.devices[0]), "hipSetDevice");
  const size_t bytes = fb.size() * sizeof(uint32_t);
  const int frames = o.frames;
  uint32_t *dev[2], *host[2];
  hipStream_t march, copy;
  hipEvent_t rendered[2], copied[2];
  ok(hipStreamCreateWithFlags(&march, hipStreamNonBlocking), "hipStreamCreate");
  ok(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking), "hipStreamCreate");
  for (int k = 0; k < 2; k++) {
    ok(hipMalloc((void **)&dev[k], bytes), "hipMalloc");
    ok(hipHostMalloc((void **)&host[k], bytes, hipHostMallocDefault), "hipHostMalloc");
    ok(hipEventCreateWithFlags(&rendered[k], hipEventDisableTiming), "hipEventCreate");
    ok(hipEventCreateWithFlags(&copied[k], hipEventDisableTiming), "hipEventCreate");
  }
  renderer.updateDt(o.dt);
  renderer.updateFrameID(0);
  renderer.render();                                   // one synchronous frame first: launch-order feedback
  const auto t1 = std::chrono::steady_clock::now();
  int accumID = 0;
  for (int fr = 0; fr < frames; fr++) {
    const int k = fr & 1;
    renderer.updateFrameID(accumID);
    if (o.pg) ++accumID;
    if (fr >= 2) ok(hipStreamWaitEvent(march, copied[k], 0), "hipStreamWaitEvent");   // buffer k has left the device
    renderer.renderAsync(dev[k], march);
    ok(hipEventRecord(rendered[k], march), "hipEventRecord");
    ok(hipStreamWaitEvent(copy, rendered[k], 0), "hipStreamWaitEvent");
    ok(hipMemcpyAsync(host[k], dev[k], bytes, hipMemcpyDeviceToHost, copy), "hipMemcpyAsync");
    ok(hipEventRecord(copied[k], copy), "hipEventRecord");
  }
  ok(hipStreamSynchronize(copy), "hipStreamSynchronize");
  ok(hipStreamSynchronize(march), "hipStreamSynchronize");
  const double secP = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
  std::memcpy(fb.data(), host[(frames - 1) & 1], bytes);
  std::printf("pipelined: %d frames in %.3f ms (%.3f ms per frame incl. copy to host)\n", frames, 1000.0 * secP, 1000.0 * secP / frames);
  for (int k = 0; k < 2; k++) { (void)hipFree(dev[k]); (void)hipHostFree(host[k]); (void)hipEventDestroy(rendered[k]); (void)hipEventDestroy(copied[k]); }
  (void)hipStreamDestroy(march); (void)hipStreamDestroy(copy);
  return renderer.stats().kernel_ms * frames;
}

// --stats, the frames, their average and the last of them as binary PPM
void renderFrames(Renderer &renderer, const FrameOpts &o, std::vector<uint32_t> &fb)
{
  if (o.stats) {       // region statistics as Regions::buildFrom prints them, and the work counters of the first frame
    renderer.updateDt(o.dt);
    renderer.updateFrameID(0);
    const ExaHipStats s = renderer.renderStats();
    std::printf("regions %zu leafEntries %zu\n", renderer.numRegions, renderer.numLeafEntries);
    std::printf("stats segments %llu samples %llu brick_visits %llu corner_loads %llu nodes_visited %llu\n", ull(s.segments), ull(s.samples),
                ull(s.brick_visits), ull(s.corner_loads), ull(s.nodes_visited));
  }
  int accumID = 0;
  double kernelMs = 0;
  const auto t0 = std::chrono::steady_clock::now();
  if (o.pipeline) kernelMs = renderPipelined(renderer, o, fb);
  else
    for (int fr = 0; fr < o.frames; fr++) {                  // viewer.cpp:279-288
      renderer.updateDt(o.dt);
      renderer.updateFrameID(accumID);
      if (o.pg) ++accumID;
      renderer.render();
      kernelMs += renderer.stats().kernel_ms;
    }
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::printf("Avg. after %d frames: %.3f FPS (%.3f ms), kernel %.3f ms\n", o.frames, o.frames / sec, 1000.0 * sec / o.frames, kernelMs / o.frames);
  if (o.outName.empty()) return;
  FILE *f = openFile(o.outName, "wb");
  std::fprintf(f, "P6\n%d %d\n255\n", o.size.x, o.size.y);
  for (int y = o.size.y - 1; y >= 0; y--)
    for (int x = 0; x < o.size.x; x++) { const uint32_t p = fb[size_t(y) * o.size.x + x]; const unsigned char rgb[3] = { (unsigned char)(p & 255), (unsigned char)((p >> 8) & 255), (unsigned char)((p >> 16) & 255) }; std::fwrite(rgb, 1, 3, f); }
  std::fclose(f);
}
} // namespace

int main(int argc, char **argv)
{
  try {
    Options o = parseOptions(argc, argv);
    FrameOpts &fo = o.frame;
    Config::SP config = Config::parseConfigFile(fo.cfgName);
    if (!config->bricks.sp) fail("no bricks file specified");
    config->bricks.sp->allowEmptyCells = fo.allowEmptyCells;
    const box3f bounds = config->getBounds();
    std::printf("bricks %zu cells %zu fields %zu\n", config->bricks.sp->numBricks(), config->bricks.sp->totalNumCells,
                config->scalarFields.size());
    for (auto &sf : config->scalarFields)
      std::printf("field %s range %.9g %.9g elements %zu\n", sf->name.c_str(), sf->valueRange.lower, sf->valueRange.upper, sf->value.size());
    std::printf("bounds %.9g %.9g %.9g  %.9g %.9g %.9g\n", bounds.lower.x, bounds.lower.y, bounds.lower.z,
                bounds.upper.x, bounds.upper.y, bounds.upper.z);
    if (fo.info) return 0;

    std::vector<uint32_t> fb(size_t(fo.size.x) * fo.size.y);
    if (fo.devices.empty()) fo.devices.push_back(0);
    Renderer renderer(config->bricks.sp, config->surfaces, config->scalarFields, fo.devices);  // viewer.cpp:1256-1260
    setupRenderer(renderer, fo, *config, bounds, fb);
    const bool anyOutput = writeOutputs(o, renderer);
    if (fo.frames == 0 && anyOutput) return 0;
    renderFrames(renderer, fo, fb);
    return 0;
  } catch (const std::exception &e) {
    std::cerr << "Fatal error " << e.what() << std::endl;
    return 1;
  }
}
