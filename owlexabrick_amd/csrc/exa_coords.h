// Which brick coordinates the float32 tables can hold (include/exa_hip.h states the rule beside ExaBrick).  Host only:
// shared by the preparation (exa_prep.cpp) and by renderer creation from a scene filled by hand (exa_create.cpp).
#pragma once
#include "../../include/exa_hip.h"

#include <cstdio>
#include <string>

namespace exa {

// Every plane the preparation and the kernels form from a brick, per axis, in double: the lower corner, the upper corner
// lower + size cw, the region-domain planes lower +- cw/2 and lower + (size +- 1/2) cw (the brick's domain reaches half a
// cell beyond its cells, the cell centres lie half a cell inside).  False, with the axis and the plane, when one of them
// is not a float32: a table built from its rounding describes another scene.  Levels are 0..30 (checked by the callers).
inline bool brickPlanesAreFloats(const ExaBrick &b, int *axis, double *plane)
{
  const double cw = double(1u << b.level);
  for (int k = 0; k < 3; k++) {
    const double lo = double(b.lower[k]), n = double(b.size[k]);
    const double planes[6] = { lo, lo - 0.5 * cw, lo + 0.5 * cw, lo + n * cw, lo + (n - 0.5) * cw, lo + (n + 0.5) * cw };
    for (double p : planes)
      if (double(float(p)) != p) { *axis = k; *plane = p; return false; }
  }
  return true;
}

inline std::string brickPlaneMessage(const char *who, uint64_t brick, const ExaBrick &b, int axis, double plane)
{
  char buf[320];
  std::snprintf(buf, sizeof buf,
                "%s: brick %llu (lower %d %d %d, size %d %d %d, level %d): its plane %c = %.17g is not a float32 "
                "(coordinates too large for the cell width)",
                who, (unsigned long long)brick, b.lower[0], b.lower[1], b.lower[2], b.size[0], b.size[1], b.size[2], b.level,
                "xyz"[axis], plane);
  return buf;
}

} // namespace exa
