// Stand-alone host check of the axis-table layout of the rectilinear lattice kernels (pynama_amd/csrc/pyn_lattice_axes.h): for every
// tile shape of PYNAMA_LATTICE_TILE, every axis length and every tile origin a launch can have -- a rank's z-slab with ghost planes
// included -- each slot the tile kernel reads (origin .. origin + T + 1, no clamping) lies inside the table and holds the coordinate
// of lattice index origin - 1 + j, or the end value where that index is off the lattice.
//   c++ -std=c++17 -fsanitize=address,undefined -I pynama_amd/csrc tools/lattice_axes_host_check.cpp -o /tmp/axes_check && /tmp/axes_check
#include <cstdio>
#include <vector>

#include "pyn_lattice_axes.h"

static long checked = 0;

// one axis: n lattice indices, tiles of T rows over the rows [first, first + rows) (first = p_own0, rows = n_own along z; 0, n else)
static bool check_axis(int n, int T, int first, int rows) {
  std::vector<double> axis(n), tab(lat_axis_slots(n));
  for (int i = 0; i < n; ++i) axis[i] = 0.5 + 3.0 * i + 0.25 * i * i;          // distinct values
  for (int s = 0; s < (int)tab.size(); ++s) tab[s] = axis.at(lat_axis_source(s, n));
  for (int origin = 0; origin < rows; origin += T)
    for (int j = 0; j < T + 2; ++j) {
      const int slot = first + origin + j, idx = first + origin - 1 + j;        // what lat_axes_load reads, what it stands for
      if (slot < 0 || slot >= (int)tab.size()) {
        std::printf("n %d T %d first %d rows %d origin %d j %d: slot %d outside [0, %zu)\n", n, T, first, rows, origin, j, slot, tab.size());
        return false;
      }
      const double want = axis[idx < 0 ? 0 : (idx >= n ? n - 1 : idx)];
      if (tab[slot] != want) {
        std::printf("n %d T %d origin %d j %d: slot %d holds %g, index %d is %g\n", n, T, origin, j, slot, tab[slot], idx, want);
        return false;
      }
      ++checked;
    }
  return true;
}

int main() {
  const int shapes[10][3] = {{7, 5, 4}, {7, 7, 7}, {6, 6, 6}, {8, 6, 6}, {7, 6, 6}, {6, 6, 4}, {6, 5, 5}, {7, 4, 4}, {14, 3, 3}, {7, 5, 5}};
  bool ok = true;
  for (const auto& sh : shapes) {
    for (int d = 0; d < 3; ++d) ok = ok && sh[d] <= LAT_AX_HI;
    for (int n = 2; n <= 70 && ok; ++n) {
      ok = ok && check_axis(n, sh[0], 0, n) && check_axis(n, sh[1], 0, n);
      for (int lo = 0; lo <= 1 && ok; ++lo)          // ghost plane below / above the owned planes of a slab
        for (int hi = 0; hi <= 1 && ok; ++hi)
          if (n - lo - hi >= 1) ok = check_axis(n, sh[2], lo, n - lo - hi);
    }
  }
  std::printf("%s: %ld table reads checked\n", ok ? "ok" : "FAILED", checked);
  return ok ? 0 : 1;
}
