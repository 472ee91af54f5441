// Stand-alone host check of the index arithmetic of the lattice rows kernel (pynama_amd/csrc/pyn_lattice_rows.h): for lattices of
// nx, ny, nz in {2, 3, 4, 9} nodes, on one rank and as a rank's z-slab at either end of the domain (a ghost plane above / below) and
// in its middle (both), every entry of every x-line's run is placed as the kernel places it (first entry of a lane by division, the further ones by lat_rows_step, the two end rows by lat_rows_end) and compared with a
// brute-force CSR graph -- the existing neighbours of every owned node sorted by node id under the slab numbering.  Checked: the
// run of line (y, zo) starts at the brute-force row offset of its first row and is lat_rows_rowptr there, every row offset equals
// lat_rows_rowptr, each entry's row, slot and neighbour are the graph's, the runs tile the value array without gap or overlap, and
// the magic division is exact for every run length a lattice of up to 2^16 nodes per line can have.
//   c++ -std=c++17 -fsanitize=address,undefined -I pynama_amd/csrc tools/lattice_rows_host_check.cpp -o /tmp/rows_check && /tmp/rows_check
#include <algorithm>
#include <cstdio>
#include <vector>

#include "pyn_lattice_rows.h"

static long checked = 0;

struct Col {
  int id, dx, dy, dz;
  bool operator<(const Col& o) const { return id < o.id; }
};

static bool check_lattice(int nx, int ny, int npl, int p_own0, int n_own) {
  std::vector<char> written;
  std::vector<int> rowptr(1, 0);
  std::vector<std::vector<Col>> rows;
  // brute force, rows in id order: owned plane zo carries the ids zo * nx * ny ..
  for (int zo = 0; zo < n_own; ++zo)
    for (int y = 0; y < ny; ++y)
      for (int x = 0; x < nx; ++x) {
        const int pl = p_own0 + zo;
        if (lat_rows_plane(nx, ny, p_own0, n_own, pl) + y * nx + x != (int)rows.size()) {
          std::printf("node (%d, %d, plane %d) is not row %zu\n", x, y, pl, rows.size());
          return false;
        }
        std::vector<Col> cols;
        for (int dz = -1; dz <= 1; ++dz)
          for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
              const int xx = x + dx, yy = y + dy, pp = pl + dz;
              if (xx < 0 || xx >= nx || yy < 0 || yy >= ny || pp < 0 || pp >= npl) continue;
              cols.push_back({lat_rows_plane(nx, ny, p_own0, n_own, pp) + yy * nx + xx, dx, dy, dz});
            }
        std::sort(cols.begin(), cols.end());
        rowptr.push_back(rowptr.back() + (int)cols.size());
        rows.push_back(cols);
      }
  written.assign(rowptr.back(), 0);
  for (int zo = 0; zo < n_own; ++zo)
    for (int y = 0; y < ny; ++y) {
      const int pl = p_own0 + zo, row0 = (zo * ny + y) * nx;
      const int zcode = lat_rows_zcode(npl, p_own0, n_own, pl);
      const int cy = 3 - (y == 0) - (y == ny - 1), cz = zcode & 3;
      const int base = lat_rows_rowptr(nx, ny, npl, p_own0, n_own, 0, y, zo), len = lat_rows_line_len(nx, cy, cz);
      const uint32_t magic = lat_rows_magic(cy * cz);
      if (base != rowptr[row0] || base + len != rowptr[row0 + nx]) {
        std::printf("%d x %d x %d (own %d + %d) line y %d zo %d: run [%d, %d), graph [%d, %d)\n", nx, ny, npl, p_own0, n_own, y, zo, base,
                    base + len, rowptr[row0], rowptr[row0 + nx]);
        return false;
      }
      for (int x = 0; x < nx; ++x)
        if (lat_rows_rowptr(nx, ny, npl, p_own0, n_own, x, y, zo) != rowptr[row0 + x]) {
          std::printf("%d x %d x %d (own %d + %d) row (%d, %d, %d): offset %d, graph %d\n", nx, ny, npl, p_own0, n_own, x, y, zo,
                      lat_rows_rowptr(nx, ny, npl, p_own0, n_own, x, y, zo), rowptr[row0 + x]);
          return false;
        }
      // one entry as the kernel places it: row x, slot group t, column offset dx
      auto entry = [&](int e, int x, int t, int dx) {
        int dy = 9, dz = 9;
        bool ok = e >= 0 && e < len && x >= 0 && x < nx && t >= 0 && t < cy * cz && !written.at(base + e);
        if (ok) {
          lat_rows_group(t, cy, y != 0, zcode, dy, dz);
          const std::vector<Col>& cols = rows.at(row0 + x);
          const int k = base + e - rowptr[row0 + x];
          ok = k >= 0 && k < (int)cols.size() && cols[k].dx == dx && cols[k].dy == dy && cols[k].dz == dz;
        }
        if (!ok) {
          std::printf("%d x %d x %d (own %d + %d) line y %d zo %d entry %d: row %d group %d neighbour (%d, %d, %d)\n", nx, ny, npl, p_own0,
                      n_own, y, zo, e, x, t, dx, dy, dz);
          return false;
        }
        written[base + e] = 1;
        ++checked;
        return true;
      };
      const int cc = cy * cz, nint = lat_rows_interior_len(nx, cc);
      for (int stride : {64, 256}) {   // (any stride walks the same entries: the kernel's is its workgroup size)
        if (stride == 256) std::fill(written.begin() + base, written.begin() + base + len, 0);
        const LatRowsStride st = lat_rows_stride(stride, cc);
        for (int lane = 0; lane < stride && lane < nint; ++lane) {
          LatRowsPos p = lat_rows_interior(lane, cc, magic);
          for (int m = lane; m < nint; m += stride) {
            if (!entry(2 * cc + m, p.x, p.t, p.kx - 1)) return false;
            lat_rows_step(p, st, cc);
          }
        }
        for (int j = 0; j < 4 * cc; ++j) {
          const LatRowsEnd r = lat_rows_end(j, nx, cc, len);
          if (!entry(r.e, r.x, r.t, r.dx)) return false;
        }
      }
    }
  for (size_t i = 0; i < written.size(); ++i)
    if (!written[i]) {
      std::printf("%d x %d x %d (own %d + %d): value %zu never written\n", nx, ny, npl, p_own0, n_own, i);
      return false;
    }
  return true;
}

// the (K1, M1) tables: rows of K1 sum to zero up to rounding, M1 sums to the axis length, missing neighbours carry nothing
static bool check_tables() {
  const int n = 9;
  double c[n], km[6], len = 0.0, ksum = 0.0;
  for (int i = 0; i < n; ++i) c[i] = 0.25 * i + 0.03125 * i * i;
  for (int i = 0; i < n; ++i) {
    lat_rows_km(c, i, n, km);
    ksum += km[0] + km[2] + km[4];
    len += km[1] + km[3] + km[5];
    if ((i == 0 && (km[0] != 0.0 || km[1] != 0.0)) || (i == n - 1 && (km[4] != 0.0 || km[5] != 0.0))) return false;
    if (i > 0 && km[0] != -1.0 / (c[i] - c[i - 1])) return false;
  }
  const double err = len - (c[n - 1] - c[0]);
  return (ksum < 0 ? -ksum : ksum) < 1e-12 && (err < 0 ? -err : err) < 1e-14;
}

int main() {
  const int sizes[4] = {2, 3, 4, 9};
  bool ok = check_tables();
  if (!ok) std::printf("1-D tables wrong\n");
  for (int nx : sizes)
    for (int ny : sizes)
      for (int nz : sizes) {
        ok = ok && check_lattice(nx, ny, nz, 0, nz);                      // one rank: every plane owned
        ok = ok && check_lattice(nx, ny, nz + 1, 0, nz);                  // the domain's bottom slab: a ghost plane above
        ok = ok && check_lattice(nx, ny, nz + 1, 1, nz);                  // the top slab: a ghost plane below
        ok = ok && check_lattice(nx, ny, nz + 2, 1, nz);                  // a middle slab: both
      }
  // e / cc by multiplication, every cc a line can have, every entry of runs up to 27 * 2^16 values
  for (int cc : {2, 3, 4, 6, 9})
    for (int e = 0; e < 27 * (1 << 16) && ok; ++e)
      if (lat_rows_div(e, lat_rows_magic(cc)) != e / cc) {
        std::printf("%d / %d by multiplication gives %d\n", e, cc, lat_rows_div(e, lat_rows_magic(cc)));
        ok = false;
      }
  std::printf("%s: %ld run entries checked\n", ok ? "ok" : "FAILED", checked);
  return ok ? 0 : 1;
}
