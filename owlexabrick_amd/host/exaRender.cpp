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
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

using namespace exa;

namespace {
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

// --derived QUANTITY: a name or a number; EXA_DERIVED_* (the module refuses an unknown number)
int derivedQuantity(const std::string &s)
{
  static const char *const names[EXA_DERIVED_QUANTITIES] = { "speed", "divergence", "vorticity", "vorticity_magnitude", "q", "helicity" };
  for (int q = 0; q < EXA_DERIVED_QUANTITIES; q++)
    if (s == names[q]) return q;
  char *end = nullptr;
  const long q = std::strtol(s.c_str(), &end, 10);
  if (end == s.c_str() || *end || q < 0) throw std::runtime_error("--derived wants speed, divergence, vorticity, vorticity_magnitude, q, helicity or a number, not " + s);
  return (int)q;
}
} // namespace

int main(int argc, char **argv)
{
  try {
    std::string cfgName, outName;
    vec2i size(600, 400);                                         // viewer default window
    vec3f vp, vi, vu;                                             // --camera
    float fov = 70.f, dt = 0.5f, xfScale = 1.f, aoLength = 1e20f;
    float isoVals[2] = { 0, 0 }; int isoChans[2] = { 0, 0 }, isoOn[2] = { 0, 0 };
    bool haveRange = false, ao = false, pg = true, skipping = true, gradDVR = true, gradISO = true, info = false, clip = false, stats = false;
    float range[2] = { 0, 1 }; box3f clipBox;
    std::string xfFile;
    int frames = 1;
    std::vector<int> devices;
    bool pipeline = false;
    bool allowEmptyCells = false;
    std::vector<float> contourPlanes;                             // 4 floats per --contourplane (normal, offset)
    std::vector<std::pair<std::string, int>> options;             // --option key=value
    std::vector<int> contourChans;
    int resampleDims[3] = { 0, 0, 0 }, resampleChannel = 0;
    std::string resampleName;
    bool resampleWorld = false, haveResampleBox = false;
    box3f resampleBox;
    float resampleFill = NAN;
    int isoDims[3] = { 0, 0, 0 }, isoChannel = 0;
    float isoValue = 0.f;
    std::string isoName;
    bool isoWorld = false, haveIsoBox = false;
    box3f isoBox;
    int histBins = 0, histChannel = 0;
    std::string histName;
    bool haveHistRange = false, haveHistBox = false;
    float histRange[2] = { 0, 1 };
    box3i histBox;
    std::string streamSeedsName, streamName;
    float streamStep = 0.f;
    int streamMaxSteps = 0;
    vec3i streamChannels(0, 1, 2);
    bool streamBoth = false, streamBackward = false, streamNormalize = false;
    std::string projectName;
    int projectChannel = 0, projectSamples = 0;
    float projectDt = 0.f;
    std::string raycastName;
    std::string surfaceName, surfaceMesh;
    std::vector<int> surfaceChannels;
    float surfaceSpacing = 0.f;
    int surfaceMaxN = 0;
    bool surfaceWorld = false;
    int raycastChannel = 0, raycastSamples = 0, raycastRefine = 0;
    float raycastIso = 0.f, raycastDt = 0.f;
    int derived = -1;                                            // --derived: EXA_DERIVED_*
    vec3i derivedChannels(0, 1, 2);
    bool haveResampleChannel = false, haveIsoChannel = false;
    std::string regionsName;
    int regionsChannel = 0, regionsDims[3] = { 0, 0, 0 };
    float regionsIso = 0.f;
    bool regionsWorld = false, regionsBelow = false, regionsFaces = false, haveRegionsBox = false;
    box3f regionsBox;
    std::string basinsName;
    int basinsChannel = 0, basinsDims[3] = { 0, 0, 0 };
    float basinsIso = 0.f, basinsMinDepth = 0.f;
    std::string linesName;
    int linesChannel = 0;
    vec3f linesOrigin, linesDu, linesDv;
    vec2i linesSize;
    std::vector<float> linesIsos;
    bool linesWorld = false;
    std::string licName;
    vec3i licChannels(0, 1, 2);
    vec3f licOrigin, licDu, licDv;
    vec2i licSize;
    float licStep = 0.5f;
    int licHalfLength = 20;
    uint32_t licSeed = 0;
    std::string criticalName;
    vec3i criticalChannels(0, 1, 2), criticalDims(2, 2, 2);
    vec3f criticalLo, criticalHi;
    int criticalIterations = 8;
    float criticalTolerance = 0.0009765625f;
    std::string ftleName;
    vec3i ftleChannels(0, 1, 2), ftleDims(1, 1, 1);
    vec3f ftleLo, ftleHi;
    float ftleStep = 0.5f;
    int ftleNumSteps = 20;
    bool ftleBackward = false;
    for (int i = 1; i < argc; i++) {
      const std::string a = argv[i];
      auto f = [&]() { if (i + 1 >= argc) throw std::runtime_error("missing value after " + a); return (float)atof(argv[++i]); };
      if (a == "--size" || a == "-win") { size.x = (int)f(); size.y = (int)f(); }
      else if (a == "--camera") { vp = { f(), f(), f() }; vi = { f(), f(), f() }; vu = { f(), f(), f() }; }
      else if (a == "--fov") fov = f();
      else if (a == "--dt") dt = f();
      else if (a == "--xf") { if (i + 1 >= argc) throw std::runtime_error("missing file after --xf"); xfFile = argv[++i]; }
      else if (a == "--xf-scale") xfScale = f();
      else if (a == "--range") { range[0] = f(); range[1] = f(); haveRange = true; }
      else if (a == "--isovals") { isoVals[0] = f(); isoVals[1] = f(); isoOn[0] = isoOn[1] = 1; }
      else if (a == "--isochans") { isoChans[0] = (int)f(); isoChans[1] = (int)f(); }
      else if (a == "--contourplane") { for (int k = 0; k < 4; k++) contourPlanes.push_back(f()); }   // viewer.cpp:1199-1205
      else if (a == "--contourchan") contourChans.push_back((int)f());                                // viewer.cpp:1206-1207
      else if (a == "--clip-box") { clipBox.lower = { f(), f(), f() }; clipBox.upper = { f(), f(), f() }; clip = true; }
      else if (a == "--ao") ao = true;
      else if (a == "--ao-length") aoLength = f();
      else if (a == "--no-pg") pg = false;
      else if (a == "--no-space-skipping") skipping = false;
      else if (a == "--gradientShadingDVR") gradDVR = f() != 0.f;
      else if (a == "--gradientShadingISO") gradISO = f() != 0.f;
      else if (a == "--frames") frames = (int)f();
      else if (a == "-o") { if (i + 1 >= argc) throw std::runtime_error("missing file after -o"); outName = argv[++i]; }
      else if (a == "--info") info = true;
      else if (a == "--stats") stats = true;
      else if (a == "--gpus") { const int n = (int)f(); devices.clear(); for (int d = 0; d < n; d++) devices.push_back(d); }
      else if (a == "--devices") {
        if (i + 1 >= argc) throw std::runtime_error("missing list after --devices");
        devices.clear();
        for (const char *p = argv[++i]; *p;) {
          char *end = nullptr;
          const long d = strtol(p, &end, 10);
          if (end == p || d < 0 || d > 1023 || (*end != ',' && *end != 0)) throw std::runtime_error("--devices wants a comma-separated list of device indices");
          devices.push_back((int)d);
          p = *end == ',' ? end + 1 : end;
          if (*end == ',' && !*p) throw std::runtime_error("--devices wants a comma-separated list of device indices");
        }
        if (devices.empty()) throw std::runtime_error("--devices wants a comma-separated list of device indices");
      }
      else if (a == "--resample") {
        for (int k = 0; k < 3; k++) resampleDims[k] = (int)f();
        if (i + 1 >= argc) throw std::runtime_error("missing file after --resample NX NY NZ");
        resampleName = argv[++i];
      }
      else if (a == "--resample-box") { resampleBox.lower = { f(), f(), f() }; resampleBox.upper = { f(), f(), f() }; haveResampleBox = true; }
      else if (a == "--resample-world") resampleWorld = true;
      else if (a == "--resample-channel") { resampleChannel = (int)f(); haveResampleChannel = true; }
      else if (a == "--resample-fill") resampleFill = f();
      else if (a == "--isomesh") {
        isoValue = f();
        for (int k = 0; k < 3; k++) isoDims[k] = (int)f();
        if (i + 1 >= argc) throw std::runtime_error("missing file after --isomesh ISO NX NY NZ");
        isoName = argv[++i];
      }
      else if (a == "--isomesh-box") { isoBox.lower = { f(), f(), f() }; isoBox.upper = { f(), f(), f() }; haveIsoBox = true; }
      else if (a == "--isomesh-world") isoWorld = true;
      else if (a == "--isomesh-channel") { isoChannel = (int)f(); haveIsoChannel = true; }
      else if (a == "--isolines") {
        linesChannel = (int)f();
        linesOrigin = { f(), f(), f() }; linesDu = { f(), f(), f() }; linesDv = { f(), f(), f() };
        linesSize.x = (int)f(); linesSize.y = (int)f();
        if (i + 2 >= argc) throw std::runtime_error("missing levels and file after --isolines CHANNEL o u v NU NV");
        for (const char *p = argv[++i]; *p;) {
          char *end = nullptr;
          const float v = std::strtof(p, &end);
          if (end == p || (*end != ',' && *end != 0)) throw std::runtime_error("--isolines wants a comma-separated list of levels");
          linesIsos.push_back(v);
          p = *end == ',' ? end + 1 : end;
        }
        linesName = argv[++i];
      }
      else if (a == "--isolines-world") linesWorld = true;
      else if (a == "--lic") {
        if (i + 1 >= argc) throw std::runtime_error("missing channels after --lic");
        char tail = 0;
        if (std::sscanf(argv[++i], "%d,%d,%d%c", &licChannels.x, &licChannels.y, &licChannels.z, &tail) != 3)
          throw std::runtime_error("--lic wants three comma-separated channels C0,C1,C2");
        licOrigin = { f(), f(), f() }; licDu = { f(), f(), f() }; licDv = { f(), f(), f() };
        licSize.x = (int)f(); licSize.y = (int)f();
        licStep = f();
        licHalfLength = (int)f();
        if (i + 1 >= argc) throw std::runtime_error("missing file after --lic C0,C1,C2 o u v NU NV STEP HALFLENGTH");
        licName = argv[++i];
      }
      else if (a == "--critical") {
        if (i + 1 >= argc) throw std::runtime_error("missing channels after --critical");
        char tail = 0;
        if (std::sscanf(argv[++i], "%d,%d,%d%c", &criticalChannels.x, &criticalChannels.y, &criticalChannels.z, &tail) != 3)
          throw std::runtime_error("--critical wants three comma-separated channels C0,C1,C2");
        criticalLo = { f(), f(), f() }; criticalHi = { f(), f(), f() };
        criticalDims.x = (int)f(); criticalDims.y = (int)f(); criticalDims.z = (int)f();
        criticalIterations = (int)f();
        criticalTolerance = f();
        if (i + 1 >= argc) throw std::runtime_error("missing file after --critical C0,C1,C2 l u NX NY NZ ITERATIONS TOLERANCE");
        criticalName = argv[++i];
      }
      else if (a == "--ftle") {
        if (i + 1 >= argc) throw std::runtime_error("missing channels after --ftle");
        char tail = 0;
        if (std::sscanf(argv[++i], "%d,%d,%d%c", &ftleChannels.x, &ftleChannels.y, &ftleChannels.z, &tail) != 3)
          throw std::runtime_error("--ftle wants three comma-separated channels C0,C1,C2");
        ftleLo = { f(), f(), f() }; ftleHi = { f(), f(), f() };
        ftleDims.x = (int)f(); ftleDims.y = (int)f(); ftleDims.z = (int)f();
        ftleStep = f();
        ftleNumSteps = (int)f();
        if (i + 2 >= argc) throw std::runtime_error("missing direction and file after --ftle C0,C1,C2 l u NX NY NZ STEP NUMSTEPS");
        const std::string dir = argv[++i];
        if (dir != "fwd" && dir != "bwd") throw std::runtime_error("--ftle wants the direction fwd or bwd");
        ftleBackward = dir == "bwd";
        ftleName = argv[++i];
      }
      else if (a == "--lic-seed") { if (i + 1 >= argc) throw std::runtime_error("missing value after --lic-seed"); licSeed = (uint32_t)std::strtoul(argv[++i], nullptr, 10); }
      else if (a == "--regions") {
        regionsChannel = (int)f();
        regionsIso = f();
        for (int k = 0; k < 3; k++) regionsDims[k] = (int)f();
        if (i + 1 >= argc) throw std::runtime_error("missing file after --regions CHANNEL ISO NX NY NZ");
        regionsName = argv[++i];
      }
      else if (a == "--basins") {
        basinsChannel = (int)f();
        basinsIso = f();
        basinsMinDepth = f();
        for (int k = 0; k < 3; k++) basinsDims[k] = (int)f();
        if (i + 1 >= argc) throw std::runtime_error("missing file after --basins CHANNEL ISO MINDEPTH NX NY NZ");
        basinsName = argv[++i];
      }
      else if (a == "--regions-box") { regionsBox.lower = { f(), f(), f() }; regionsBox.upper = { f(), f(), f() }; haveRegionsBox = true; }
      else if (a == "--regions-world") regionsWorld = true;
      else if (a == "--regions-below") regionsBelow = true;
      else if (a == "--regions-faces") regionsFaces = true;
      else if (a == "--derived") {
        if (i + 1 >= argc) throw std::runtime_error("missing quantity after --derived");
        derived = derivedQuantity(argv[++i]);
        derivedChannels.x = (int)f(); derivedChannels.y = (int)f(); derivedChannels.z = (int)f();
      }
      else if (a == "--histogram") {
        histBins = (int)f();
        if (i + 1 >= argc) throw std::runtime_error("missing file after --histogram BINS");
        histName = argv[++i];
      }
      else if (a == "--histogram-channel") histChannel = (int)f();
      else if (a == "--histogram-range") { histRange[0] = f(); histRange[1] = f(); haveHistRange = true; }
      else if (a == "--histogram-box") {
        auto n = [&]() { if (i + 1 >= argc) throw std::runtime_error("missing value after " + a); return (int)std::strtol(argv[++i], nullptr, 10); };
        histBox.lower = { n(), n(), n() }; histBox.upper = { n(), n(), n() }; haveHistBox = true;
      }
      else if (a == "--streamlines") {
        if (i + 1 >= argc) throw std::runtime_error("missing seed file after --streamlines");
        streamSeedsName = argv[++i];
        streamStep = f();
        streamMaxSteps = (int)f();
        if (i + 1 >= argc) throw std::runtime_error("missing file after --streamlines SEEDS.txt STEP MAXSTEPS");
        streamName = argv[++i];
      }
      else if (a == "--streamlines-channels") { streamChannels.x = (int)f(); streamChannels.y = (int)f(); streamChannels.z = (int)f(); }
      else if (a == "--streamlines-both") streamBoth = true;
      else if (a == "--streamlines-backward") streamBackward = true;
      else if (a == "--streamlines-normalize") streamNormalize = true;
      else if (a == "--project") {
        projectChannel = (int)f();
        projectDt = f();
        projectSamples = (int)f();
        if (i + 1 >= argc) throw std::runtime_error("missing file after --project CHANNEL DT NSAMPLES");
        projectName = argv[++i];
      }
      else if (a == "--raycast") {
        raycastChannel = (int)f();
        raycastIso = f();
        raycastDt = f();
        raycastSamples = (int)f();
        raycastRefine = (int)f();
        if (i + 1 >= argc) throw std::runtime_error("missing file after --raycast CHANNEL ISO DT NSAMPLES REFINE");
        raycastName = argv[++i];
      }
      else if (a == "--surface") {
        if (i + 2 >= argc) throw std::runtime_error("missing mesh and channels after --surface");
        surfaceMesh = argv[++i];
        for (const char *c = argv[++i]; *c;) {
          char *end = nullptr;
          surfaceChannels.push_back((int)std::strtol(c, &end, 10));
          if (end == c || (*end && *end != ',')) throw std::runtime_error("--surface: channels are C0[,C1,C2,C3]");
          c = *end ? end + 1 : end;
        }
        surfaceSpacing = f();
        surfaceMaxN = (int)f();
        if (i + 1 >= argc) throw std::runtime_error("missing file after --surface MESH CHANNELS SPACING MAXN");
        surfaceName = argv[++i];
      }
      else if (a == "--surface-world") surfaceWorld = true;
      else if (a == "--pipeline") pipeline = true;
      else if (a == "--allow-empty-cells") allowEmptyCells = true;    // the reference built with -DALLOW_EMPTY_CELLS=1
      else if (a == "--option") {                                     // exa_hip_set_option: --option walk=2, --option ao_overlap=0 ...
        if (i + 1 >= argc) throw std::runtime_error("missing key=value after --option");
        const std::string kv = argv[++i];
        const size_t eq = kv.find('=');
        char *end = nullptr;
        const long v = eq == std::string::npos ? 0 : std::strtol(kv.c_str() + eq + 1, &end, 10);
        if (eq == std::string::npos || eq == 0 || end == kv.c_str() + eq + 1 || *end) throw std::runtime_error("--option wants key=integer");
        options.emplace_back(kv.substr(0, eq), (int)v);
      }
      else if (a[0] != '-') cfgName = a;
      else throw std::runtime_error("unknown flag " + a);
    }
    if (cfgName.empty()) throw std::runtime_error("usage: exaRender cfg.exa [flags]");
    if (derived != -1 && (haveResampleChannel || haveIsoChannel))
      throw std::runtime_error("--derived takes its three channels itself: --resample-channel / --isomesh-channel do not go with it");
    Config::SP config = Config::parseConfigFile(cfgName);
    if (!config->bricks.sp) throw std::runtime_error("no bricks file specified");
    config->bricks.sp->allowEmptyCells = allowEmptyCells;
    const box3f bounds = config->getBounds();
    std::printf("bricks %zu cells %zu fields %zu\n", config->bricks.sp->numBricks(), config->bricks.sp->totalNumCells,
                config->scalarFields.size());
    for (auto &sf : config->scalarFields)
      std::printf("field %s range %.9g %.9g elements %zu\n", sf->name.c_str(), sf->valueRange.lower, sf->valueRange.upper, sf->value.size());
    std::printf("bounds %.9g %.9g %.9g  %.9g %.9g %.9g\n", bounds.lower.x, bounds.lower.y, bounds.lower.z,
                bounds.upper.x, bounds.upper.y, bounds.upper.z);
    if (info) return 0;

    std::vector<uint32_t> fb(size_t(size.x) * size.y);
    if (devices.empty()) devices.push_back(0);
    Renderer renderer(config->bricks.sp, config->surfaces, config->scalarFields, devices);  // viewer.cpp:1256-1260
    for (const auto &kv : options) renderer.setOption(kv.first, kv.second);
    if (devices.size() > 1) std::printf("devices %zu\n", devices.size());
    renderer.setVoxelSpaceTransform(config->bricks.voxelSpaceTransform);
    renderer.resizeFrameBuffer(fb.data(), size);
    if (vu != vec3f(0.f)) setupCamera(renderer, vp, vi, vu, fov, size);
    else setupCamera(renderer, bounds.center() + vec3f(-.3f, .7f, 1.f) * bounds.span(), bounds.center(), vec3f(0, 1, 0), 70.f, size);

    // default transfer function: alpha ramp, grey ramp colour (the PNG colormaps are UI assets)
    std::vector<float> alpha(NUM_XF_VALUES);
    std::vector<vec3f> color(NUM_XF_VALUES);
    for (int i = 0; i < NUM_XF_VALUES; i++) { alpha[i] = i / float(NUM_XF_VALUES - 1); color[i] = vec3f(alpha[i]); }
    if (!xfFile.empty()) {                                          // 128 raw floats (viewer.cpp:139-145,1147-1152)
      FILE *f = std::fopen(xfFile.c_str(), "rb");
      if (!f || std::fread(alpha.data(), sizeof(float), NUM_XF_VALUES, f) != (size_t)NUM_XF_VALUES) throw std::runtime_error("cannot read " + xfFile);
      std::fclose(f);
    }
    for (size_t c = 0; c < config->scalarFields.size(); c++) {      // viewer.cpp:567-575
      interval<float> dom = config->scalarFields[c]->valueRange;
      if (haveRange) dom = interval<float>(range[0], range[1]);
      renderer.updateXF((int)c, alpha.data(), color, dom, xfScale);
    }
    renderer.updateIsoValues(isoVals, isoChans, isoOn);
    if (!contourPlanes.empty()) {
      // the viewer's contour panel set-up (viewer.cpp:673-690): planes given on the command line are enabled, the
      // others keep their defaults (axis i % 3, offset .5, off); the channels apply when more than one was given
      vec3f n[MAX_CONTOUR_PLANES]; float off[MAX_CONTOUR_PLANES]; int ch[MAX_CONTOUR_PLANES], en[MAX_CONTOUR_PLANES];
      if (contourPlanes.size() / 4 > (size_t)MAX_CONTOUR_PLANES) throw std::runtime_error("too many contour planes");
      for (int i = 0; i < MAX_CONTOUR_PLANES; i++) {
        if (contourPlanes.size() / 4 > (size_t)i) {
          n[i] = vec3f(contourPlanes[4 * i], contourPlanes[4 * i + 1], contourPlanes[4 * i + 2]);
          off[i] = contourPlanes[4 * i + 3]; en[i] = 1;
        } else {
          n[i] = vec3f(i % 3 == 0 ? 1.f : 0.f, i % 3 == 1 ? 1.f : 0.f, i % 3 == 2 ? 1.f : 0.f);
          off[i] = .5f; en[i] = 0;
        }
        ch[i] = (contourChans.size() > 1 && (size_t)i < contourChans.size()) ? contourChans[i] : 0;
      }
      renderer.updateContourPlanes(n, off, ch, en);
    }
    renderer.setSpaceSkipping(skipping);
    renderer.setGradientShadingDVR(gradDVR);
    renderer.setGradientShadingISO(gradISO);
    renderer.frameState.ao.enabled = ao;                            // viewer.cpp:944-959
    renderer.frameState.ao.length = aoLength;
    renderer.frameState.clipBox.enabled = clip;
    if (clip) {
      const box3f wb = renderer.worldSpaceBounds;
      renderer.frameState.clipBox.coords.lower = wb.lower + clipBox.lower * wb.span();
      renderer.frameState.clipBox.coords.upper = wb.lower + clipBox.upper * wb.span();
    }
    if (!resampleName.empty()) {
      const box3f box = haveResampleBox ? resampleBox : (resampleWorld ? renderer.worldSpaceBounds : renderer.voxelSpaceBounds);
      const vec3i dims(resampleDims[0], resampleDims[1], resampleDims[2]);
      if (dims.x < 1 || dims.y < 1 || dims.z < 1) throw std::runtime_error("--resample wants NX NY NZ >= 1");
      const size_t comps = derived == EXA_DERIVED_VORTICITY ? 3 : 1;
      std::vector<float> grid(size_t(dims.x) * size_t(dims.y) * size_t(dims.z) * comps);
      // sampled with a NaN fill to count the points outside every region (a reconstructed value is never NaN for a field
      // without NaNs), then the requested fill written in their place
      if (derived < 0) renderer.resample(box, dims, resampleChannel, grid.data(), resampleWorld, NAN);
      else renderer.resampleDerived(box, dims, derivedChannels, derived, grid.data(), resampleWorld, NAN);
      size_t invalid = 0;                                             // floats: `comps` per lattice point
      for (float &v : grid)
        if (std::isnan(v)) { v = resampleFill; invalid++; }
      FILE *f = std::fopen(resampleName.c_str(), "wb");
      if (!f || std::fwrite(grid.data(), sizeof(float), grid.size(), f) != grid.size()) throw std::runtime_error("cannot write " + resampleName);
      std::fclose(f);
      std::printf("resample %d %d %d box %.9g %.9g %.9g %.9g %.9g %.9g ", dims.x, dims.y, dims.z,
                  box.lower.x, box.lower.y, box.lower.z, box.upper.x, box.upper.y, box.upper.z);
      if (derived < 0) std::printf("channel %d invalid %zu\n", resampleChannel, invalid);
      else std::printf("derived %d channels %d %d %d components %zu invalid %zu\n", derived, derivedChannels.x, derivedChannels.y,
                       derivedChannels.z, comps, invalid);
    }
    size_t isoTriangles = 0;
    if (!isoName.empty()) {
      const box3f box = haveIsoBox ? isoBox : (isoWorld ? renderer.worldSpaceBounds : renderer.voxelSpaceBounds);
      const vec3i dims(isoDims[0], isoDims[1], isoDims[2]);
      const bool keep = surfaceMesh == "iso";          // --surface iso reads the module's copy
      TriangleMesh::SP mesh = derived < 0 ? renderer.extractIsoSurface(box, dims, isoChannel, isoValue, isoWorld, nullptr, keep)
                                          : renderer.extractIsoSurfaceDerived(box, dims, derivedChannels, derived, isoValue, isoWorld, keep);
      isoTriangles = mesh->index.size();
      TriangleMesh::save(isoName, { mesh });
      std::printf("isomesh %d %d %d box %.9g %.9g %.9g %.9g %.9g %.9g ", dims.x, dims.y, dims.z, box.lower.x, box.lower.y,
                  box.lower.z, box.upper.x, box.upper.y, box.upper.z);
      if (derived < 0) std::printf("channel %d ", isoChannel);
      else std::printf("derived %d channels %d %d %d ", derived, derivedChannels.x, derivedChannels.y, derivedChannels.z);
      std::printf("iso %.9g vertices %zu triangles %zu\n", isoValue, mesh->vertex.size(), mesh->index.size());
    }
    if (!linesName.empty()) {
      const Renderer::Isolines L = derived < 0 ? renderer.isolines(linesOrigin, linesDu, linesDv, linesSize, linesIsos, linesChannel, linesWorld)
                                               : renderer.isolinesDerived(linesOrigin, linesDu, linesDv, linesSize, linesIsos, derivedChannels, derived, linesWorld);
      FILE *f = std::fopen(linesName.c_str(), "wb");
      if (!f) throw std::runtime_error("cannot write " + linesName);
      const size_t n = linesIsos.size(), nv = L.vertex.size(), ns = L.segment.size() / 2;
      std::fprintf(f, "isolines %d %d levels %zu vertices %zu segments %zu\n", linesSize.x, linesSize.y, n, nv, ns);
      const bool ok = std::fwrite(linesIsos.data(), 4, n, f) == n && std::fwrite(L.vertexOffsets.data(), 8, n + 1, f) == n + 1
                   && std::fwrite(L.segmentOffsets.data(), 8, n + 1, f) == n + 1 && std::fwrite(L.vertex.data(), 12, nv, f) == nv
                   && std::fwrite(L.uv.data(), 8, nv, f) == nv && std::fwrite(L.segment.data(), 8, ns, f) == ns;
      if (std::fclose(f) || !ok) throw std::runtime_error("cannot write " + linesName);
      std::printf("isolines %d %d ", linesSize.x, linesSize.y);
      if (derived < 0) std::printf("channel %d ", linesChannel);
      else std::printf("derived %d channels %d %d %d ", derived, derivedChannels.x, derivedChannels.y, derivedChannels.z);
      std::printf("world %d levels %zu vertices %zu segments %zu\n", linesWorld ? 1 : 0, n, nv, ns);
    }
    if (!licName.empty()) {
      const Renderer::Lic L = renderer.lic(licOrigin, licDu, licDv, licSize, licChannels, licStep, licHalfLength, nullptr, licSeed);
      FILE *f = std::fopen(licName.c_str(), "wb");
      if (!f) throw std::runtime_error("cannot write " + licName);
      const size_t n = L.lic.size();
      std::fprintf(f, "lic %d %d channels %d %d %d step %.9g halfLength %d seed %u\n", licSize.x, licSize.y, licChannels.x, licChannels.y,
                   licChannels.z, licStep, licHalfLength, licSeed);
      const bool ok = std::fwrite(L.lic.data(), 4, n, f) == n;
      if (std::fclose(f) || !ok) throw std::runtime_error("cannot write " + licName);
      size_t covered = 0;
      unsigned long long samples = 0;
      for (uint32_t c : L.count) { covered += c > 0; samples += c; }
      std::printf("lic %d %d channels %d %d %d step %.9g halfLength %d seed %u pixels_covered %zu samples %llu\n", licSize.x, licSize.y,
                  licChannels.x, licChannels.y, licChannels.z, licStep, licHalfLength, licSeed, covered, samples);
    }
    if (!ftleName.empty()) {
      const Renderer::Flowmap M = renderer.flowmap(ftleLo, ftleHi, ftleDims, ftleChannels, ftleStep, ftleNumSteps, ftleBackward);
      FILE *f = std::fopen(ftleName.c_str(), "wb");
      if (!f) throw std::runtime_error("cannot write " + ftleName);
      const size_t n = M.stretch.size();
      std::fprintf(f, "ftle %d %d %d channels %d %d %d step %.9g numSteps %d direction %s\n", ftleDims.x, ftleDims.y, ftleDims.z,
                   ftleChannels.x, ftleChannels.y, ftleChannels.z, ftleStep, ftleNumSteps, ftleBackward ? "bwd" : "fwd");
      const bool ok = std::fwrite(M.end.data(), 12, n, f) == n && std::fwrite(M.steps.data(), 4, n, f) == n
                      && std::fwrite(M.reason.data(), 4, n, f) == n && std::fwrite(M.stretch.data(), 4, n, f) == n
                      && std::fwrite(M.ftle.data(), 4, n, f) == n;
      if (std::fclose(f) || !ok) throw std::runtime_error("cannot write " + ftleName);
      size_t valid = 0;
      for (float v : M.ftle) valid += !std::isnan(v);
      std::printf("ftle %d %d %d channels %d %d %d step %.9g numSteps %d direction %s points_with_ftle %zu\n", ftleDims.x, ftleDims.y,
                  ftleDims.z, ftleChannels.x, ftleChannels.y, ftleChannels.z, ftleStep, ftleNumSteps, ftleBackward ? "bwd" : "fwd", valid);
    }
    if (!criticalName.empty()) {
      const Renderer::CriticalPoints P = renderer.criticalPoints(box3f(criticalLo, criticalHi), criticalDims, criticalChannels,
                                                                 criticalIterations, criticalTolerance);
      FILE *f = std::fopen(criticalName.c_str(), "wb");
      if (!f) throw std::runtime_error("cannot write " + criticalName);
      const ExaHipCriticalStats &st = P.stats;
      char line[512];
      std::snprintf(line, sizeof(line), "critical %d %d %d box %.9g %.9g %.9g %.9g %.9g %.9g channels %d %d %d iterations %d tolerance %.9g "
                    "cells %llu invalidCells %llu candidates %llu found %llu nonFinite %llu leftCell %llu notConverged %llu",
                    criticalDims.x, criticalDims.y, criticalDims.z, criticalLo.x, criticalLo.y, criticalLo.z, criticalHi.x, criticalHi.y,
                    criticalHi.z, criticalChannels.x, criticalChannels.y, criticalChannels.z, criticalIterations, criticalTolerance,
                    (unsigned long long)st.cells, (unsigned long long)st.invalidCells, (unsigned long long)st.candidates,
                    (unsigned long long)st.found, (unsigned long long)st.nonFinite, (unsigned long long)st.leftCell,
                    (unsigned long long)st.notConverged);
      std::fprintf(f, "%s\n", line);
      const size_t n = P.points.size();
      const bool ok = std::fwrite(P.points.data(), sizeof(ExaHipCriticalPoint), n, f) == n;
      if (std::fclose(f) || !ok) throw std::runtime_error("cannot write " + criticalName);
      // the found points by n+ (sink, the two saddles, source) and, of each, the spiralling ones
      size_t kind[4] = { 0, 0, 0, 0 }, spiral[4] = { 0, 0, 0, 0 }, degenerate = 0;
      for (const ExaHipCriticalPoint &p : P.points) {
        kind[p.type & 3]++;
        spiral[p.type & 3] += (p.type & EXA_CRITICAL_SPIRAL) ? 1 : 0;
        degenerate += (p.type & EXA_CRITICAL_DEGENERATE) ? 1 : 0;
      }
      std::printf("%s sinks %zu spiral %zu saddles1 %zu spiral %zu saddles2 %zu spiral %zu sources %zu spiral %zu degenerate %zu\n", line,
                  kind[0], spiral[0], kind[1], spiral[1], kind[2], spiral[2], kind[3], spiral[3], degenerate);
    }
    if (!regionsName.empty()) {
      const box3f box = haveRegionsBox ? regionsBox : (regionsWorld ? renderer.worldSpaceBounds : renderer.voxelSpaceBounds);
      const vec3i dims(regionsDims[0], regionsDims[1], regionsDims[2]);
      const Renderer::Regions R = derived < 0 ? renderer.regions(box, dims, regionsChannel, regionsIso, regionsWorld, regionsBelow, regionsFaces)
                                              : renderer.regionsDerived(box, dims, derivedChannels, derived, regionsIso, regionsWorld, regionsBelow, regionsFaces);
      FILE *f = std::fopen(regionsName.c_str(), "wb");
      if (!f) throw std::runtime_error("cannot write " + regionsName);
      const size_t nr = R.regions.size(), n = R.labels.size();
      std::fprintf(f, "regions %d %d %d count %zu inside %llu exponent %d\n", dims.x, dims.y, dims.z, nr,
                   (unsigned long long)R.numInside, R.sumExponent);
      const bool ok = std::fwrite(R.regions.data(), sizeof(ExaHipRegion), nr, f) == nr && std::fwrite(R.labels.data(), 4, n, f) == n;
      if (std::fclose(f) || !ok) throw std::runtime_error("cannot write " + regionsName);
      std::printf("regions %d %d %d ", dims.x, dims.y, dims.z);
      if (derived < 0) std::printf("channel %d ", regionsChannel);
      else std::printf("derived %d channels %d %d %d ", derived, derivedChannels.x, derivedChannels.y, derivedChannels.z);
      std::printf("iso %.9g world %d below %d faces %d count %zu inside %llu exponent %d\n", regionsIso, regionsWorld ? 1 : 0,
                  regionsBelow ? 1 : 0, regionsFaces ? 1 : 0, nr, (unsigned long long)R.numInside, R.sumExponent);
    }
    if (!basinsName.empty()) {
      const box3f box = haveRegionsBox ? regionsBox : (regionsWorld ? renderer.worldSpaceBounds : renderer.voxelSpaceBounds);
      const vec3i dims(basinsDims[0], basinsDims[1], basinsDims[2]);
      const Renderer::Basins B = derived < 0 ? renderer.basins(box, dims, basinsChannel, basinsIso, basinsMinDepth, regionsWorld, regionsBelow, regionsFaces)
                                             : renderer.basinsDerived(box, dims, derivedChannels, derived, basinsIso, basinsMinDepth, regionsWorld, regionsBelow, regionsFaces);
      FILE *f = std::fopen(basinsName.c_str(), "wb");
      if (!f) throw std::runtime_error("cannot write " + basinsName);
      const size_t nb = B.basins.size(), n = B.labels.size();
      std::fprintf(f, "basins %d %d %d count %zu raw %llu rounds %d inside %llu exponent %d\n", dims.x, dims.y, dims.z, nb,
                   (unsigned long long)B.numRaw, B.rounds, (unsigned long long)B.numInside, B.sumExponent);
      const bool ok = std::fwrite(B.basins.data(), sizeof(ExaHipBasin), nb, f) == nb && std::fwrite(B.labels.data(), 4, n, f) == n;
      if (std::fclose(f) || !ok) throw std::runtime_error("cannot write " + basinsName);
      std::printf("basins %d %d %d ", dims.x, dims.y, dims.z);
      if (derived < 0) std::printf("channel %d ", basinsChannel);
      else std::printf("derived %d channels %d %d %d ", derived, derivedChannels.x, derivedChannels.y, derivedChannels.z);
      std::printf("iso %.9g minDepth %.9g world %d below %d faces %d count %zu raw %llu rounds %d inside %llu exponent %d\n", basinsIso,
                  basinsMinDepth, regionsWorld ? 1 : 0, regionsBelow ? 1 : 0, regionsFaces ? 1 : 0, nb, (unsigned long long)B.numRaw, B.rounds,
                  (unsigned long long)B.numInside, B.sumExponent);
    }
    if (!surfaceName.empty()) {
      const bool fromIso = surfaceMesh == "iso";
      if (fromIso && isoName.empty()) throw std::runtime_error("--surface iso needs --isomesh in the same invocation");
      Renderer::SurfaceSamples S;
      const bool world = fromIso ? isoWorld : surfaceWorld;
      if (fromIso) S = renderer.sampleIsoSurface(isoTriangles, surfaceChannels.data(), (int)surfaceChannels.size(), surfaceSpacing, surfaceMaxN, world);
      else {
        TriangleMesh all;                                // the file's meshes as one
        for (const TriangleMesh::SP &m : TriangleMesh::load(surfaceMesh)) {
          const int base = (int)all.vertex.size();
          all.vertex.insert(all.vertex.end(), m->vertex.begin(), m->vertex.end());
          for (const vec3i &t : m->index) all.index.push_back(vec3i(t.x + base, t.y + base, t.z + base));
        }
        S = renderer.sampleTriangles(all, surfaceChannels.data(), (int)surfaceChannels.size(), surfaceSpacing, surfaceMaxN, world);
      }
      const Renderer::SurfaceIntegrals I = Renderer::surfaceIntegrals(S);
      const size_t nt = S.subdiv.size(), nc = surfaceChannels.size();
      FILE *f = std::fopen(surfaceName.c_str(), "wb");
      if (!f) throw std::runtime_error("cannot write " + surfaceName);
      std::fprintf(f, "surface triangles %zu channels %zu", nt, nc);
      for (int c : surfaceChannels) std::fprintf(f, " %d", c);
      std::fprintf(f, " spacing %.9g maxN %d world %d\n", surfaceSpacing, surfaceMaxN, world ? 1 : 0);
      for (size_t t = 0; t < nt; t++) {
        std::fprintf(f, "%d %.9g %.9g %.9g %.17g", S.subdiv[t], S.areaNormal[t].x, S.areaNormal[t].y, S.areaNormal[t].z, I.area[t]);
        for (size_t c = 0; c < nc; c++)
          std::fprintf(f, " %u %.17g %.17g %.17g", S.count[t * nc + c], S.sum[t * nc + c], I.mean[t * nc + c], I.integral[t * nc + c]);
        std::fprintf(f, "\n");
      }
      std::fprintf(f, "invalid %llu\n", (unsigned long long)I.invalidTriangles);
      for (size_t c = 0; c < nc; c++)
        std::fprintf(f, "total %d covered_area %.17g uncovered_area %.17g uncovered_triangles %llu integral %.17g force %.17g %.17g %.17g\n",
                     surfaceChannels[c], I.coveredArea[c], I.uncoveredArea[c], (unsigned long long)I.uncoveredTriangles[c],
                     I.totalIntegral[c], I.force[3 * c], I.force[3 * c + 1], I.force[3 * c + 2]);
      if (nc == 3) std::fprintf(f, "flux %.17g\n", I.flux);
      if (std::fclose(f)) throw std::runtime_error("cannot write " + surfaceName);
      std::printf("surface triangles %zu channels %zu spacing %.9g maxN %d invalid %llu\n", nt, nc, surfaceSpacing, surfaceMaxN,
                  (unsigned long long)I.invalidTriangles);
    }
    if (!histName.empty()) {
      if (histBins < 1) throw std::runtime_error("--histogram wants BINS >= 1");
      const box3i *box = haveHistBox ? &histBox : nullptr;
      interval<float> range(histRange[0], histRange[1]);
      if (!haveHistRange) {
        const ExaHipFieldStats r = renderer.fieldStats(histChannel, box);
        if (!(r.min < r.max)) throw std::runtime_error("--histogram: the field is constant (or has no value) there: give --histogram-range lo hi");
        range = interval<float>(r.min, r.max);
      }
      std::vector<uint64_t> cells, volume;
      ExaHipFieldStats st;
      renderer.computeHistogram(histChannel, range, histBins, cells, &volume, &st, box);
      FILE *f = std::fopen(histName.c_str(), "w");
      if (!f) throw std::runtime_error("cannot write " + histName);
      for (size_t b = 0; b < cells.size(); b++) std::fprintf(f, "%llu %llu\n", (unsigned long long)cells[b], (unsigned long long)volume[b]);
      if (std::fclose(f)) throw std::runtime_error("cannot write " + histName);
      std::printf("histogram channel %d bins %d range %.9g %.9g slots %llu empty %llu nan %llu under %llu over %llu binned %llu\n", histChannel,
                  histBins, range.lower, range.upper, (unsigned long long)st.slots, (unsigned long long)st.empty, (unsigned long long)st.nan,
                  (unsigned long long)st.under, (unsigned long long)st.over, (unsigned long long)st.binned);
    }
    if (!streamName.empty()) {
      std::vector<vec3f> seeds;
      FILE *f = std::fopen(streamSeedsName.c_str(), "r");
      if (!f) throw std::runtime_error("cannot read " + streamSeedsName);
      char word[3][64];
      int got;
      while ((got = std::fscanf(f, "%63s %63s %63s", word[0], word[1], word[2])) == 3)     // strtof: nan and inf are seeds too
        seeds.push_back(vec3f(std::strtof(word[0], nullptr), std::strtof(word[1], nullptr), std::strtof(word[2], nullptr)));
      std::fclose(f);
      if (got != EOF) throw std::runtime_error(streamSeedsName + ": a seed is three numbers `x y z`");
      const Renderer::Streamlines L = renderer.streamlines(seeds.data(), seeds.size(), streamChannels, streamStep, streamMaxSteps,
                                                           streamBoth || !streamBackward, streamBoth || streamBackward, streamNormalize);
      f = std::fopen(streamName.c_str(), "w");
      if (!f) throw std::runtime_error("cannot write " + streamName);
      for (size_t i = 0; i < seeds.size(); i++) {
        std::fprintf(f, "%u %d %d %llu", L.seedVertex[i], L.reason[2 * i], L.reason[2 * i + 1], (unsigned long long)(L.offset[i + 1] - L.offset[i]));
        for (uint64_t v = L.offset[i]; v < L.offset[i + 1]; v++) std::fprintf(f, " %.9g %.9g %.9g", L.vertex[v].x, L.vertex[v].y, L.vertex[v].z);
        std::fprintf(f, "\n");
      }
      if (std::fclose(f)) throw std::runtime_error("cannot write " + streamName);
      std::printf("streamlines seeds %zu channels %d %d %d step %.9g maxSteps %d vertices %zu\n", seeds.size(), streamChannels.x,
                  streamChannels.y, streamChannels.z, streamStep, streamMaxSteps, L.vertex.size());
    }
    if (!projectName.empty()) {
      const ExaHipRays rays = renderer.cameraRays(size, 0.f, projectDt, projectSamples);
      const Renderer::Projection P = renderer.project(rays, projectChannel, true, true);
      std::vector<float> integral(P.sum.size());
      size_t hit = 0;
      for (size_t k = 0; k < integral.size(); k++) { integral[k] = float(P.sum[k] * double(projectDt)); hit += P.count[k] != 0; }
      FILE *f = std::fopen(projectName.c_str(), "wb");
      if (!f) throw std::runtime_error("cannot write " + projectName);
      std::fprintf(f, "project %d %d channel %d dt %.9g samples %d\n", size.x, size.y, projectChannel, projectDt, projectSamples);
      const size_t n = integral.size();
      const bool ok = std::fwrite(integral.data(), 4, n, f) == n && std::fwrite(P.count.data(), 4, n, f) == n
                   && std::fwrite(P.max.data(), 4, n, f) == n && std::fwrite(P.min.data(), 4, n, f) == n;
      if (std::fclose(f) || !ok) throw std::runtime_error("cannot write " + projectName);
      std::printf("project %d %d channel %d dt %.9g samples %d pixels_hit %zu\n", size.x, size.y, projectChannel, projectDt,
                  projectSamples, hit);
    }
    if (!raycastName.empty()) {
      const ExaHipRays rays = renderer.cameraRays(size, 0.f, raycastDt, raycastSamples);
      const Renderer::IsoHits R = renderer.raycastIso(rays, raycastChannel, raycastIso, raycastRefine, true, true);
      FILE *f = std::fopen(raycastName.c_str(), "wb");
      if (!f) throw std::runtime_error("cannot write " + raycastName);
      std::fprintf(f, "raycast %d %d channel %d iso %.9g dt %.9g samples %d refine %d\n", size.x, size.y, raycastChannel, raycastIso,
                   raycastDt, raycastSamples, raycastRefine);
      const size_t n = R.t.size();
      const bool ok = std::fwrite(R.t.data(), 4, n, f) == n && std::fwrite(R.position.data(), 12, n, f) == n
                   && std::fwrite(R.value.data(), 4, n, f) == n && std::fwrite(R.gradient.data(), 12, n, f) == n
                   && std::fwrite(R.index.data(), 4, n, f) == n && std::fwrite(R.side.data(), 4, n, f) == n
                   && std::fwrite(R.crossings.data(), 4, n, f) == n;
      if (std::fclose(f) || !ok) throw std::runtime_error("cannot write " + raycastName);
      size_t hit = 0;
      for (int32_t k : R.index) hit += k >= 0;
      std::printf("raycast %d %d channel %d iso %.9g dt %.9g samples %d refine %d pixels_hit %zu\n", size.x, size.y, raycastChannel,
                  raycastIso, raycastDt, raycastSamples, raycastRefine, hit);
    }
    if (frames == 0 && (!resampleName.empty() || !isoName.empty() || !histName.empty() || !streamName.empty() || !projectName.empty()
                        || !raycastName.empty() || !surfaceName.empty() || !linesName.empty() || !regionsName.empty() || !basinsName.empty()
                        || !licName.empty() || !ftleName.empty() || !criticalName.empty())) return 0;
    if (stats) {       // region statistics as Regions::buildFrom prints them, and the work counters of the first frame
      renderer.updateDt(dt);
      renderer.updateFrameID(0);
      const ExaHipStats s = renderer.renderStats();
      std::printf("regions %zu leafEntries %zu\n", renderer.numRegions, renderer.numLeafEntries);
      std::printf("stats segments %llu samples %llu brick_visits %llu corner_loads %llu nodes_visited %llu\n",
                  (unsigned long long)s.segments, (unsigned long long)s.samples, (unsigned long long)s.brick_visits,
                  (unsigned long long)s.corner_loads, (unsigned long long)s.nodes_visited);
    }
    int accumID = 0;
    double kernelMs = 0;
    const auto t0 = std::chrono::steady_clock::now();
    if (!pipeline) {
      for (int fr = 0; fr < frames; fr++) {                          // viewer.cpp:279-288
        renderer.updateDt(dt);
        renderer.updateFrameID(accumID);
        if (pg) ++accumID;
        renderer.render();
        kernelMs += renderer.stats().kernel_ms;
      }
    } else {
      // two device frames + two pinned host frames: the march of frame k+1 runs while frame k travels to the host
      auto ok = [](hipError_t e, const char *what) { if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e)); };
      ok(hipSetDevice(devices[0]), "hipSetDevice");
      const size_t bytes = fb.size() * sizeof(uint32_t);
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
      renderer.updateDt(dt);
      renderer.updateFrameID(0);
      renderer.render();                                   // one synchronous frame first: launch-order feedback
      const auto t1 = std::chrono::steady_clock::now();
      for (int fr = 0; fr < frames; fr++) {
        const int k = fr & 1;
        renderer.updateFrameID(accumID);
        if (pg) ++accumID;
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
      kernelMs = renderer.stats().kernel_ms * frames;
      std::printf("pipelined: %d frames in %.3f ms (%.3f ms per frame incl. copy to host)\n", frames, 1000.0 * secP, 1000.0 * secP / frames);
      for (int k = 0; k < 2; k++) { (void)hipFree(dev[k]); (void)hipHostFree(host[k]); (void)hipEventDestroy(rendered[k]); (void)hipEventDestroy(copied[k]); }
      (void)hipStreamDestroy(march); (void)hipStreamDestroy(copy);
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("Avg. after %d frames: %.3f FPS (%.3f ms), kernel %.3f ms\n", frames, frames / sec, 1000.0 * sec / frames, kernelMs / frames);
    if (!outName.empty()) {
      FILE *f = std::fopen(outName.c_str(), "wb");
      if (!f) throw std::runtime_error("cannot write " + outName);
      std::fprintf(f, "P6\n%d %d\n255\n", size.x, size.y);
      for (int y = size.y - 1; y >= 0; y--)
        for (int x = 0; x < size.x; x++) { const uint32_t p = fb[size_t(y) * size.x + x]; const unsigned char rgb[3] = { (unsigned char)(p & 255), (unsigned char)((p >> 8) & 255), (unsigned char)((p >> 16) & 255) }; std::fwrite(rgb, 1, 3, f); }
      std::fclose(f);
    }
    return 0;
  } catch (const std::exception &e) {
    std::cerr << "Fatal error " << e.what() << std::endl;
    return 1;
  }
}
