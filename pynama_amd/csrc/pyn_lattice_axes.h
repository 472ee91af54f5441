// Layout of the axis tables of a rectilinear lattice (LatArgs::axX / axY / axZ, pyn_lattice.h): plain C++, no device code, so that
// the stand-alone host check (tools/lattice_axes_host_check.cpp) includes exactly what the kernels index with.
#pragma once

#if defined(__HIPCC__)
#define PYN_AX_HD __host__ __device__
#else
#define PYN_AX_HD
#endif

// Guard slots of an axis table below index 0 and above index n - 1 (copies of the end values): a tile reads the T + 2 entries of
// its node box -- lattice indices origin - 1 .. origin + T, i.e. slots origin .. origin + T + 1 -- without clamping, and the last
// tile of an axis may start at index n - 1 (tiles up to LAT_AX_HI rows wide).
constexpr int LAT_AX_LO = 1, LAT_AX_HI = 16;
PYN_AX_HD inline int lat_axis_slots(int n) { return n + LAT_AX_LO + LAT_AX_HI; }
PYN_AX_HD inline int lat_axis_source(int slot, int n) {   // lattice index whose coordinate table slot `slot` holds
  const int i = slot - LAT_AX_LO;
  return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}
