// Stand-alone host check of the index arithmetic of the lattice rows kernel (pynama_amd/csrc/pyn_lattice_rows.h): for lattices of
// nx, ny, nz in {2, 3, 4, 9} nodes, on one rank and as a rank's z-slab at either end of the domain (a ghost plane above / below) and
// in its middle (both), every entry of every x-line's run is placed as the kernel places it (first entry of a lane by division, the further ones by lat_rows_step, the two end rows by lat_rows_end) and compared with a
// brute-force CSR graph -- the existing neighbours of every owned node sorted by node id under the slab numbering.  Checked: the
// run of line (y, zo) starts at the brute-force row offset of its first row and is lat_rows_rowptr there, every row offset equals
// lat_rows_rowptr, each entry's row, slot and neighbour are the graph's, the runs tile the value array without gap or overlap, and
// the magic division is exact for every run length a lattice of up to 2^16 nodes per line can have.  For the persistent form: the
// schedule (check_sched) for grids of 1, 2, 3, 7, 8, 9, 64 and 2048 workgroups over 1 .. 5000 lines, and the word of every line
// (check_classes) on lattices up to 6 x 5 x 4 nodes under structured Dirichlet sets and a seeded sample.
//   c++ -std=c++17 -fsanitize=address,undefined -I pynama_amd/csrc tools/lattice_rows_host_check.cpp -o /tmp/rows_check && /tmp/rows_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
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

// The persistent form's schedule (lat_rows_sched): for `grid` workgroups and n lines every line is visited exactly once, a workgroup's
// trips end with its first -1, and the lines of the workgroups that share an XCD (wg mod 8) form one contiguous range.
static long sched_checked = 0;
static bool check_sched(int grid, int n) {
  std::vector<int> seen(n, 0), lo(8, n), hi(8, -1), cnt(8, 0);
  for (int wg = 0; wg < grid; ++wg) {
    int trip = 0, prev = -1;
    for (;; ++trip) {
      const int line = lat_rows_sched(wg, grid, n, trip);
      if (line < 0) break;
      if (line >= n || line <= prev) {
        std::printf("schedule: grid %d, %d lines: workgroup %d trip %d -> line %d after %d\n", grid, n, wg, trip, line, prev);
        return false;
      }
      prev = line;
      ++seen[line];
      const int j = wg & 7;
      lo[j] = std::min(lo[j], line);
      hi[j] = std::max(hi[j], line);
      ++cnt[j];
      ++sched_checked;
    }
    for (int extra = trip; extra < trip + 3; ++extra)   // "none" stays "none"
      if (lat_rows_sched(wg, grid, n, extra) >= 0) {
        std::printf("schedule: grid %d, %d lines: workgroup %d has a line after its last\n", grid, n, wg);
        return false;
      }
  }
  for (int l = 0; l < n; ++l)
    if (seen[l] != 1) {
      std::printf("schedule: grid %d, %d lines: line %d visited %d times\n", grid, n, l, seen[l]);
      return false;
    }
  for (int j = 0; j < 8; ++j)
    if (cnt[j] && hi[j] - lo[j] + 1 != cnt[j]) {
      std::printf("schedule: grid %d, %d lines: XCD %d holds %d lines out of [%d, %d]\n", grid, n, j, cnt[j], lo[j], hi[j]);
      return false;
    }
  return true;
}

// The word of a line (lat_rows_line_bits / lat_rows_word, as lattice_rows_map_kernel builds it) against a brute-force statement of
// its class: over ALL nodes of the lattice, the imposed ones within one line of (y, plane) in y and z decide -- none: 0, at x = 0 /
// x = nx - 1 only: 1, else 2.  For classes 0 and 1 every flag the kernel takes out of the word (lat_rows_word_flag) must be the
// node's.  unsafe: a class-2 line reported as 0 or 1 (wrong matrix); slow: a class 0 / 1 line reported as 2 (merely slow).
static long cls_checked = 0, cls_unsafe = 0, cls_slow = 0, cls_hist[3] = {0, 0, 0};
static bool check_classes(int nx, int ny, int npl, int p_own0, int n_own, const std::vector<char>& imposed) {   // imposed[(pl ny + y) nx + x]
  auto at = [&](int x, int y, int pl) { return imposed[((size_t)pl * ny + y) * nx + x] != 0; };
  for (int zo = 0; zo < n_own; ++zo)
    for (int y = 0; y < ny; ++y) {
      const int pl = p_own0 + zo, zcode = lat_rows_zcode(npl, p_own0, n_own, pl);
      uint32_t bits = 0;
      for (int lane = 0; lane < 4; ++lane)   // partial results of several lanes, OR-ed, as the kernel does
        bits |= lat_rows_line_bits(nx, ny, y, zcode, lane, 4, [&](int dy, int dz, int x) { return at(x, y + dy, pl + dz); });
      const uint32_t word = lat_rows_word(bits);
      int brute = 0;
      for (int pp = 0; pp < npl; ++pp)
        for (int yy = 0; yy < ny; ++yy)
          for (int x = 0; x < nx; ++x)
            if (at(x, yy, pp) && std::abs(yy - y) <= 1 && std::abs(pp - pl) <= 1) brute = std::max(brute, x == 0 || x == nx - 1 ? 1 : 2);
      const int got = lat_rows_class(word);
      ++cls_checked;
      ++cls_hist[brute];
      if (brute == 2 && got != 2) ++cls_unsafe;
      if (brute != 2 && got == 2) ++cls_slow;
      if (got != brute) {
        std::printf("class: %d x %d x %d (own %d + %d) line y %d zo %d: word says %d, brute force %d\n", nx, ny, npl, p_own0, n_own, y, zo, got, brute);
        return false;
      }
      if (got == 2) continue;
      const int cy = 3 - (y == 0) - (y == ny - 1), cc = cy * (zcode & 3);
      for (int t = 0; t < cc; ++t) {
        int dy, dz;
        lat_rows_group(t, cy, y != 0, zcode, dy, dz);
        for (int x = -1; x <= nx; ++x) {
          const bool want = x >= 0 && x < nx && at(x, y + dy, pl + dz);
          if ((lat_rows_word_flag(word, t, x, nx) != 0) != want) {
            std::printf("class: %d x %d x %d line y %d zo %d group %d node %d: flag out of the word %u\n", nx, ny, npl, y, zo, t, x,
                        lat_rows_word_flag(word, t, x, nx));
            return false;
          }
        }
      }
    }
  return true;
}

static bool check_all_classes() {
  uint64_t rng = 0x9e3779b97f4a7c15ull;   // seeded: the sample is the same in every run
  auto next = [&]() {
    rng ^= rng << 13;
    rng ^= rng >> 7;
    rng ^= rng << 17;
    return rng;
  };
  bool ok = true;
  for (int nx = 2; nx <= 6 && ok; ++nx)
    for (int ny = 1; ny <= 5 && ok; ++ny)
      for (int nz = 1; nz <= 4 && ok; ++nz)
        for (int slab = 0; slab < 4 && ok; ++slab) {   // one rank, a ghost plane above, below, both
          if ((ny == 1 || nz == 1) && slab) continue;
          const int p_own0 = slab >= 2 ? 1 : 0, npl = nz + (slab == 1 || slab == 2) + 2 * (slab == 3), nn = nx * ny * npl;
          auto node = [&](int x, int y, int pl) { return ((size_t)pl * ny + y) * nx + x; };
          std::vector<std::vector<char>> sets;
          sets.emplace_back(nn, 0);                                          // none
          std::vector<char> faces(nn, 0), face(nn, 0);
          for (int pl = 0; pl < npl; ++pl)
            for (int y = 0; y < ny; ++y)
              for (int x = 0; x < nx; ++x) {
                faces[node(x, y, pl)] = x == 0 || x == nx - 1 || y == 0 || y == ny - 1 || pl == 0 || pl == npl - 1;
                face[node(x, y, pl)] = x == 0;
              }
          sets.push_back(faces);                                             // all faces
          sets.push_back(face);                                              // one face (x = 0) ...
          for (auto& f : face) f = 0;
          for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) face[node(x, y, npl - 1)] = 1;
          sets.push_back(face);                                              // ... and the top one (a ghost plane in a slab)
          for (int x : {nx / 2, 1, nx - 2, 0, nx - 1}) {                     // a single node: interior, x = 1, x = nx - 2, the two ends
            std::vector<char> one(nn, 0);
            one[node(x, ny / 2, npl / 2)] = 1;
            sets.push_back(one);
            std::vector<char> ghost(nn, 0);                                  // ... and on the last plane only
            ghost[node(x, ny - 1, npl - 1)] = 1;
            sets.push_back(ghost);
          }
          for (int k = 0; k < 24; ++k) {                                     // the seeded sample, sparse to dense
            std::vector<char> r(nn, 0);
            for (auto& f : r) f = next() % 16 < (uint64_t)(1 + k % 8);
            if (k % 3 == 0)                                                  // ... and ends-only sets, so that class 1 is well sampled
              for (int i = 0; i < nn; ++i) r[i] = r[i] && (i % nx == 0 || i % nx == nx - 1);
            sets.push_back(r);
          }
          for (const auto& s : sets) ok = ok && check_classes(nx, ny, npl, p_own0, nz, s);
        }
  return ok;
}

int main() {
  const int sizes[4] = {2, 3, 4, 9};
  bool ok = check_tables();
  if (!ok) std::printf("1-D tables wrong\n");
  for (int grid : {1, 2, 3, 7, 8, 9, 64, 2048}) {
    for (int n = 1; n <= 300 && ok; ++n) ok = ok && check_sched(grid, n);
    for (int n : {511, 512, 513, 1000, 2047, 2048, 2049, 3001, 4099, 5000})
      ok = ok && check_sched(grid, n);
  }
  ok = ok && check_all_classes();
  ok = ok && cls_unsafe == 0;
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
  std::printf("%s: %ld run entries checked, %ld scheduled trips, %ld line classes (%ld / %ld / %ld of class 0 / 1 / 2; class 2 reported lower: %ld, "
              "class 0 or 1 reported as 2: %ld)\n",
              ok ? "ok" : "FAILED", checked, sched_checked, cls_checked, cls_hist[0], cls_hist[1], cls_hist[2], cls_unsafe, cls_slow);
  return ok ? 0 : 1;
}
