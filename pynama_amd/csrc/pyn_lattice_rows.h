// Index arithmetic of a box lattice's CSR rows and of the x-line kernel that streams them (assemble_q1_lattice_rows_kernel,
// pyn_assemble_lattice.hip): plain C++, no device code, so that the stand-alone host check (tools/lattice_rows_host_check.cpp)
// includes exactly what the kernels index with.  A lattice is nx x ny nodes per plane and npl local planes, of which the planes
// [p_own0, p_own0 + n_own) are owned (a rank's z-slab; one rank: all of them).
#pragma once
#include <cstdint>

#include "pyn_lattice_axes.h"

// First node id of z-plane j under the slab numbering: the owned planes carry the ids 0 .. n_own - 1 in z order, the ghost planes
// below them follow, then the ghost planes above (on one rank simply j * nx * ny).
PYN_AX_HD inline int lat_rows_plane(int nx, int ny, int p_own0, int n_own, int j) {
  const int pp = nx * ny, lo = p_own0, hi = p_own0 + n_own;
  if (j < lo) return (n_own + j) * pp;
  if (j >= hi) return (n_own + lo + (j - hi)) * pp;
  return (j - lo) * pp;
}

// z-order code of OWNED plane pl: count | the (dz + 1) of the existing z-neighbours sorted by node id, two bits each from bit 2 --
// owned planes first (ascending), then the ghost plane below, then the ghost plane above
PYN_AX_HD inline int lat_rows_zcode(int npl, int p_own0, int n_own, int pl) {
  const int lo = p_own0, hi = p_own0 + n_own;
  const bool has_dn = pl > 0, has_up = pl < npl - 1;
  const bool dn_ghost = has_dn && pl - 1 < lo, up_ghost = has_up && pl + 1 >= hi;
  int code = 0, n = 0;
  if (has_dn && !dn_ghost) code |= 0 << (2 + 2 * n++);
  code |= 1 << (2 + 2 * n++);
  if (has_up && !up_ghost) code |= 2 << (2 + 2 * n++);
  if (dn_ghost) code |= 0 << (2 + 2 * n++);
  if (up_ghost) code |= 2 << (2 + 2 * n++);
  return code | n;
}

// CSR offset of the row of owned node (x, y, owned plane zo): rows in id order, len = cx cy cz with c = 3 minus the domain faces the
// node sits on (a slab interface is not a face: its ghost plane supplies the columns); sum_{x' < x} cx(x') = 3x - (x > 0), sum over
// a whole line = 3 nx - 2.
PYN_AX_HD inline int lat_rows_rowptr(int nx, int ny, int npl, int p_own0, int n_own, int x, int y, int zo) {
  const int sx = 3 * nx - 2, sy = 3 * ny - 2;
  const bool bot = p_own0 == 0, top = p_own0 + n_own == npl;   // does the slab hold the domain's end planes?
  const int cy = 3 - (y == 0) - (y == ny - 1), cz = 3 - (bot && zo == 0) - (top && zo == n_own - 1);
  return (3 * zo - (bot && zo > 0)) * sy * sx + cz * ((3 * y - (y > 0)) * sx + cy * (3 * x - (x > 0)));
}

// ---- one x-line (y, owned plane): its nx rows are ONE run of cy cz (3 nx - 2) values, cy / cz the y / z neighbours that exist
PYN_AX_HD inline int lat_rows_line_len(int nx, int cy, int cz) { return cy * cz * (3 * nx - 2); }

// e / cc without a division: q = (e * magic) >> 32 with magic = ceil(2^32 / cc) is exact while e (cc - 1) < 2^32; cc = cy cz is one
// of 4, 6, 9 and a run has fewer than 27 nx entries
PYN_AX_HD inline uint32_t lat_rows_magic(int cc) { return (uint32_t)((0x100000000ull + (uint32_t)cc - 1) / (uint32_t)cc); }
PYN_AX_HD inline int lat_rows_div(int e, uint32_t magic) { return (int)(((uint64_t)(uint32_t)e * magic) >> 32); }

// Where a run entry sits.  CSR slot k of row x is k = t cx + kx with the slot group t = kz cy + ky (the neighbouring x-line: its
// (dy, dz) by lat_rows_group, the same for every row of the line) and kx counting the cx = 3 - (x == 0) - (x == nx - 1) columns of
// that line next to x -- the slot layout of lat_store_rows (pyn_lattice.h), columns sorted by node id.
struct LatRowsPos {
  int x, t, kx;
};

// slot group t of line y (y_inner = (y != 0)) in a plane with z code zcode -> the neighbouring line (y + dy, plane + dz)
PYN_AX_HD inline void lat_rows_group(int t, int cy, int y_inner, int zcode, int& dy, int& dz) {
  const int kz = (t >= cy) + (t >= 2 * cy);
  dy = t - kz * cy - y_inner;
  dz = ((zcode >> (2 + 2 * kz)) & 3) - 1;
}

// The rows x = 1 .. nx - 2 all have cx = 3: they are the entries [2 cc, len - 2 cc) of the run, and entry 2 cc + m is
// m = ((x - 1) cc + t) 3 + kx with dx = kx - 1.  A lane finds its first entry by division (once per line) ...
PYN_AX_HD inline int lat_rows_interior_len(int nx, int cc) { return (nx - 2) * 3 * cc; }
PYN_AX_HD inline LatRowsPos lat_rows_interior(int m, int cc, uint32_t magic) {
  const int g = m / 3, q = lat_rows_div(g, magic);
  LatRowsPos p;
  p.x = q + 1;
  p.t = g - q * cc;
  p.kx = m - 3 * g;
  return p;
}
// ... and every further one, `stride` entries on, by additions and two conditional corrections (no division, no multiplication in
// the store loop): stride = 3 (qs cc + rs) + ks
struct LatRowsStride {
  int ks, qs, rs;
};
PYN_AX_HD inline LatRowsStride lat_rows_stride(int stride, int cc) {
  LatRowsStride s;
  s.ks = stride % 3;
  s.qs = (stride / 3) / cc;
  s.rs = (stride / 3) % cc;
  return s;
}
PYN_AX_HD inline void lat_rows_step(LatRowsPos& p, const LatRowsStride& s, int cc) {
  p.kx += s.ks;
  const int c1 = p.kx >= 3;          // (kx <= 4: one correction)
  p.kx -= c1 ? 3 : 0;
  p.t += s.rs + c1;
  const int c2 = p.t >= cc;          // (t <= 2 cc - 1: one correction)
  p.t -= c2 ? cc : 0;
  p.x += s.qs + c2;
}

// The two end rows x = 0 and x = nx - 1 have cx = 2: entries [0, 2 cc) and [len - 2 cc, len), slot k = 2 t + kx.  j in [0, 4 cc)
// numbers them; `e` is the entry of the run, dx the column's offset.
struct LatRowsEnd {
  int e, x, t, dx;
};
PYN_AX_HD inline LatRowsEnd lat_rows_end(int j, int nx, int cc, int len) {
  const int last = j >= 2 * cc, jj = j - (last ? 2 * cc : 0);
  LatRowsEnd r;
  r.e = last ? len - 2 * cc + jj : jj;
  r.x = last ? nx - 1 : 0;
  r.t = jj >> 1;
  r.dx = (jj & 1) - last;
  return r;
}

// ---- the persistent form: `grid` workgroups walk the n x-lines (line = zo ny + y).  Workgroups are dealt round-robin to the 8 XCDs,
// so the workgroups wg = j (mod 8) form group j and share one L2; group j owns ONE contiguous range of lines -- the range
// xcd_contiguous_tile (pyn_lattice.h) gives it when there is a workgroup per line -- and inside it workgroup w of the group's g takes
// the lines w, w + g, w + 2 g, ..: the group's store front stays a narrow moving window.  Fewer than 8 workgroups: as many groups.
// Returns the line of workgroup wg's trip, -1 when it has none left.
PYN_AX_HD inline int lat_rows_sched(int wg, int grid, int n, int trip) {
  const int ng = grid < 8 ? grid : 8, j = wg % ng, w = wg / ng;
  const int g = (grid - j + ng - 1) / ng;                       // workgroups of group j
  const int q = n / ng, r = n % ng, cnt = q + (j < r);          // its lines: [lo, lo + cnt)
  const int64_t i = w + (int64_t)trip * g;
  return i < cnt ? j * q + (j < r ? j : r) + (int)i : -1;
}

// ---- a word per line for the current Dirichlet set (lattice_rows_map_kernel): what the <= 9 neighbouring x-lines, the line itself
// included, impose.  An imposed node at x of the line behind slot group t sets bit 2 + t (x = 0), bit 11 + t (x = nx - 1) or bit 31
// (any other x); the word is these bits with the class in bits 0-1 (bit 31 dropped):
//   0: no imposed node -- 1: imposed nodes at x = 0 and x = nx - 1 only -- 2: anything else.
// In classes 0 and 1 the rows x = 2 .. nx - 3 meet no flag (their columns lie in 1 .. nx - 2), and every flag the other four rows
// meet is a bit of the word: such a line loads no flag byte at all.
PYN_AX_HD inline uint32_t lat_rows_node_bits(int x, int nx, int t, bool imposed) {
  return !imposed ? 0u : x == 0 ? 1u << (2 + t) : x == nx - 1 ? 1u << (11 + t) : 1u << 31;
}
// the bits of the nodes x = x0, x0 + xstep, .. of every neighbouring line of line y in a plane with z code zcode;
// imposed(dy, dz, x): is node x of the line (y + dy, plane + dz) imposed?  (partial results of several callers are OR-ed)
template <class F>
PYN_AX_HD inline uint32_t lat_rows_line_bits(int nx, int ny, int y, int zcode, int x0, int xstep, F imposed) {
  const int cy = 3 - (y == 0) - (y == ny - 1), cc = cy * (zcode & 3);
  uint32_t bits = 0;
  for (int t = 0; t < cc; ++t) {
    int dy, dz;
    lat_rows_group(t, cy, y != 0, zcode, dy, dz);
    for (int x = x0; x < nx; x += xstep) bits |= lat_rows_node_bits(x, nx, t, imposed(dy, dz, x));
  }
  return bits;
}
PYN_AX_HD inline uint32_t lat_rows_word(uint32_t bits) { return (bits & 0x7ffffffcu) | ((bits >> 31) ? 2u : bits ? 1u : 0u); }
PYN_AX_HD inline int lat_rows_class(uint32_t word) { return (int)(word & 3u); }
// class 0 / 1: is node xx of the line behind slot group t imposed?
PYN_AX_HD inline unsigned lat_rows_word_flag(uint32_t word, int t, int xx, int nx) {
  return xx == 0 ? (word >> (2 + t)) & 1u : xx == nx - 1 ? (word >> (11 + t)) & 1u : 0u;
}

// ---- the 1-D P1 tables behind the values: per axis and node i six doubles, (K1[i][d], M1[i][d]) for the neighbour d - 1 = -1, 0, +1,
//   K1[i] = (-1/h[i-1], 1/h[i-1] + 1/h[i], -1/h[i]),  M1[i] = (h[i-1]/6, (h[i-1] + h[i])/3, h[i]/6),  h[i] = |c[i+1] - c[i]|,
// the terms of a missing neighbour dropped.  They follow the three axis tables in one buffer, x | y | z (z by plane position in the
// slab, ghost planes included), from an even offset: a (K1, M1) pair is one 16-byte load.
PYN_AX_HD inline int lat_rows_tab_base(int nx, int ny, int npl) {
  return (lat_axis_slots(nx) + lat_axis_slots(ny) + lat_axis_slots(npl) + 1) & ~1;
}
PYN_AX_HD inline int lat_rows_tab_doubles(int nx, int ny, int npl) { return 6 * (nx + ny + npl); }
// c: the axis' coordinates, c[i] for lattice index i in [0, n)
PYN_AX_HD inline void lat_rows_km(const double* c, int i, int n, double* km) {
  const bool lo = i > 0, hi = i < n - 1;
  double hm = lo ? c[i] - c[i - 1] : 0.0, hp = hi ? c[i + 1] - c[i] : 0.0;
  hm = hm < 0.0 ? -hm : hm;
  hp = hp < 0.0 ? -hp : hp;
  const double rm = lo ? 1.0 / hm : 0.0, rp = hi ? 1.0 / hp : 0.0;
  km[0] = -rm;
  km[1] = hm / 6.0;
  km[2] = rm + rp;
  km[3] = (hm + hp) / 3.0;
  km[4] = -rp;
  km[5] = hp / 6.0;
}
