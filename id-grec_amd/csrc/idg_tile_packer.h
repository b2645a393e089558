// Length-balanced packing of SpMM work units into tiles (host code only: no HIP here, so the library and a
// stand-alone test program compile the same text).
//
// The dense tile kernel gives one workgroup to a tile; its lane groups (BLOCK / (d/4): 32 / 16 / 8 / 4 at
// d = 32 / 64 / 128 / 256) draw the tile's virtual rows in list order and walk each in rounds of `unroll` entries.  A
// tile holds its wave slots until its LAST lane group is done, so a lane group is busy for
//     sum of the vrows' rounds / (groups x makespan of the list schedule)
// of the tile's life.  Consecutive rows packed to an entry cap score ~0.38 on power-law degree lists: a tile of ~15
// vrows for 16 groups lasts as long as its longest vrow.  Here a tile is filled with units of SIMILAR length up to
// groups x R rounds, R = rounds of its longest vrow (at least `min_rounds`, so that staging is amortised): every
// lane group then has R rounds of work.
//
// A unit is a plain vrow (nseg = 1) or a split row's whole run of segments (nseg = 2..lslots: it needs nseg LDS
// partial slots and goes into one tile whole).  Which units share a tile is free: no result depends on it.
//
// Deterministic: the packing is a function of the unit list and the limits alone (stable counting sort by length,
// one sequential fill per band; the bands are independent of each other and may be packed by concurrent threads).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace idg_pack {

struct Limits {
  int tile_nnz = 1024;   // entries a tile may stage
  int lslots = 8;        // LDS partial slots = segments of split rows per tile
  int tile_vrows = 256;  // vrows per tile
  int groups = 16;       // lane groups the fill aims at (d = 64)
  int unroll = 8;        // entries per round of a walk
  int min_rounds = 8;    // shortest tile life aimed at, in rounds
};

// What the library packs the dense launches' second schedule with (idg_graph.hip; the tile kernel stages up to 1024
// entries, 8 partial slots and 256 vrows).  Measured on the yelp2018 shape (history/balanced-tiles.md): the launch is
// fastest with ~512-entry tiles that live ~4 rounds, not with the fullest tiles.
inline Limits dense_limits() {
  Limits lim;
  lim.tile_nnz = 512;
  lim.min_rounds = 4;
  return lim;
}

struct Unit {
  int32_t len;   // entries of the unit (all its segments together); one longer than tile_nnz gets a tile of its own
  int32_t seg;   // entries of its longest vrow: the segment length (len when nseg == 1)
  int16_t nseg;  // 1: plain vrow; 2..lslots: the segments of a split row (all `seg` long but the last)
  int16_t band;  // placement band: a tile's units all come from one band
};

struct Packing {
  std::vector<int32_t> order;       // unit ids tile after tile; longest first inside a tile
  std::vector<int64_t> tile_begin;  // n_tiles + 1 offsets into `order`
  int64_t n_tiles() const { return tile_begin.empty() ? 0 : (int64_t)tile_begin.size() - 1; }
};

inline int64_t rounds_of(int64_t len, int unroll) { return std::max<int64_t>(1, (len + unroll - 1) / unroll); }

// rounds of all the vrows of a unit
inline int64_t unit_rounds(const Unit& u, int unroll) {
  if (u.nseg <= 1) return rounds_of(u.len, unroll);
  return (int64_t)(u.nseg - 1) * rounds_of(u.seg, unroll) + rounds_of(u.len - (int64_t)(u.nseg - 1) * u.seg, unroll);
}

// Makespan, in rounds, of vrows of the given lengths drawn in list order by `groups` lane groups (each group takes
// the next vrow when it finishes its own): what a tile's life is, staging aside.
template <typename LenAt>
inline int64_t list_makespan(int64_t n_vrows, LenAt len_at, int groups, int unroll) {
  std::vector<int64_t> busy((size_t)std::max(groups, 1), 0);
  for (int64_t v = 0; v < n_vrows; ++v) {
    size_t g = 0;
    for (size_t q = 1; q < busy.size(); ++q)
      if (busy[q] < busy[g]) g = q;
    busy[g] += rounds_of(len_at(v), unroll);
  }
  return *std::max_element(busy.begin(), busy.end());
}

// Packs the units of ONE band (ids[0..n), in ascending id order) and appends the tiles to `out`.
inline void pack_band(const Unit* units, const int32_t* ids, int64_t n, const Limits& lim, Packing* out) {
  if (out->tile_begin.empty()) out->tile_begin.push_back(0);
  if (n <= 0) return;
  // buckets by the rounds of the unit's longest vrow; split rows (class 0) and plain vrows (class 1) apart, because
  // only the former compete for LDS slots.  Stable: inside a bucket the ids ascend.
  int64_t max_r = 1;
  for (int64_t i = 0; i < n; ++i) max_r = std::max(max_r, rounds_of(units[ids[i]].seg, lim.unroll));
  const size_t nb = (size_t)max_r + 1;
  std::vector<int64_t> start[2] = {std::vector<int64_t>(nb + 1, 0), std::vector<int64_t>(nb + 1, 0)};
  for (int64_t i = 0; i < n; ++i) {
    const Unit& u = units[ids[i]];
    ++start[u.nseg > 1 ? 0 : 1][(size_t)rounds_of(u.seg, lim.unroll) + 1];
  }
  for (int c = 0; c < 2; ++c)
    for (size_t r = 0; r < nb; ++r) start[c][r + 1] += start[c][r];
  std::vector<int32_t> sorted[2] = {std::vector<int32_t>((size_t)start[0][nb]), std::vector<int32_t>((size_t)start[1][nb])};
  {
    std::vector<int64_t> fill[2] = {start[0], start[1]};
    for (int64_t i = 0; i < n; ++i) {
      const Unit& u = units[ids[i]];
      const int c = u.nseg > 1 ? 0 : 1;
      sorted[c][(size_t)fill[c][(size_t)rounds_of(u.seg, lim.unroll)]++] = ids[i];
    }
  }
  std::vector<int64_t> cur[2] = {start[0], start[1]};  // next unit of bucket r: sorted[c][cur[c][r]], up to start[c][r + 1]
  auto left = [&](int c, int64_t r) { return start[c][(size_t)r + 1] - cur[c][(size_t)r]; };
  int64_t top = max_r;  // no bucket above `top` has units left
  int64_t remaining = n;
  while (remaining > 0) {
    while (top > 1 && left(0, top) == 0 && left(1, top) == 0) --top;
    const int64_t R = std::max<int64_t>(top, lim.min_rounds);
    const int64_t budget = (int64_t)lim.groups * R;
    const int64_t cap = lim.tile_nnz;
    int64_t nnz = 0, vrows = 0, slots = 0, rounds = 0;
    const size_t first = out->order.size();
    for (int64_t r = top; r >= 1; --r) {
      for (int c = 0; c < 2; ++c) {
        while (left(c, r) > 0) {
          const int32_t id = sorted[c][(size_t)cur[c][(size_t)r]];
          const Unit& u = units[id];
          const int64_t ur = unit_rounds(u, lim.unroll);
          const bool seed = out->order.size() == first;  // a tile takes its first unit whatever its size
          const bool fits = nnz + u.len <= cap && vrows + u.nseg <= lim.tile_vrows &&
                            (u.nseg <= 1 || slots + u.nseg <= lim.lslots) && rounds + ur <= budget;
          if (!seed && !fits) break;
          out->order.push_back(id);
          ++cur[c][(size_t)r];
          --remaining;
          nnz += u.len, vrows += u.nseg, rounds += ur;
          if (u.nseg > 1) slots += u.nseg;
        }
      }
      if (nnz >= cap || vrows >= lim.tile_vrows || rounds >= budget) break;
    }
    // longest first inside the tile: by vrow length, then by unit length; ties keep the order of the fill
    std::stable_sort(out->order.begin() + (std::ptrdiff_t)first, out->order.end(), [&](int32_t a, int32_t b) {
      const Unit &x = units[a], &y = units[b];
      const int64_t rx = rounds_of(x.seg, lim.unroll), ry = rounds_of(y.seg, lim.unroll);
      return rx != ry ? rx > ry : x.len > y.len;
    });
    out->tile_begin.push_back((int64_t)out->order.size());
  }
}

// All bands, band 0 first.  `n_bands` = 1 + the largest band id in use.
inline void pack(const Unit* units, int64_t n, int n_bands, const Limits& lim, Packing* out) {
  out->order.clear();
  out->tile_begin.assign(1, 0);
  out->order.reserve((size_t)n);
  std::vector<std::vector<int32_t>> ids((size_t)std::max(n_bands, 1));
  for (int64_t i = 0; i < n; ++i) ids[(size_t)units[i].band].push_back((int32_t)i);
  for (const auto& b : ids) pack_band(units, b.data(), (int64_t)b.size(), lim, out);
}

struct Stats {
  int64_t tiles = 0, rounds = 0, slots = 0;  // slots = sum over tiles of groups x makespan
};

// rounds and lane-group slots of a packing (utilisation = rounds / slots)
inline Stats stats_of(const Unit* units, const Packing& p, const Limits& lim) {
  Stats s;
  s.tiles = p.n_tiles();
  std::vector<int64_t> lens;
  for (int64_t t = 0; t < s.tiles; ++t) {
    lens.clear();
    for (int64_t i = p.tile_begin[(size_t)t]; i < p.tile_begin[(size_t)t + 1]; ++i) {
      const Unit& u = units[p.order[(size_t)i]];
      for (int q = 0; q < u.nseg; ++q)
        lens.push_back(u.nseg <= 1 ? u.len : (q + 1 < u.nseg ? u.seg : u.len - (int64_t)(u.nseg - 1) * u.seg));
    }
    for (int64_t l : lens) s.rounds += rounds_of(l, lim.unroll);
    s.slots += (int64_t)lim.groups * list_makespan((int64_t)lens.size(), [&](int64_t v) { return lens[(size_t)v]; }, lim.groups, lim.unroll);
  }
  return s;
}

}  // namespace idg_pack
