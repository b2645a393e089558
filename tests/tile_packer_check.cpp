// Stand-alone check of the length-balanced tile packer (id-grec_amd/csrc/idg_tile_packer.h), built with
// -fsanitize=address,undefined by tests/test_tile_packer.py.
//
//   tile_packer_check [FILE min_utilisation]...
//
// Built-in degree lists (edge-case lengths, an all-equal list, one giant row) are always run; every FILE holds one
// more: "n_rows" then one "length band" pair per row.  For each list and each kernel width the program packs twice
// and asserts: identical results, every unit in exactly one tile, every limit, band purity, a split row's segments
// adjacent; for FILEs (at 16 lane groups) also the utilisation bound and "no more tiles than the consecutive packing".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "idg_tile_packer.h"

namespace {

using idg_pack::Limits;
using idg_pack::Packing;
using idg_pack::Unit;

#define CHECK(c, ...)                                 \
  do {                                                \
    if (!(c)) {                                       \
      std::fprintf(stderr, "FAILED %s: ", #c);        \
      std::fprintf(stderr, __VA_ARGS__);              \
      std::fprintf(stderr, "\n");                     \
      std::exit(1);                                   \
    }                                                 \
  } while (0)

struct Row {
  int64_t len;
  int band;
};

// the library's split rule, restated (idg_graph.hip: rows of more than 128 entries are cut into segments of
// max(64, ~sqrt(len)) entries, at most 8 per 512-entry chunk; each chunk is one unit)
int64_t seg_len_for(int64_t len) {
  int64_t s = (int64_t)std::ceil(std::sqrt((double)len));
  s = (s + 7) / 8 * 8;
  return std::min<int64_t>(std::max<int64_t>(s, 64), 1024);
}

std::vector<Unit> units_of(const std::vector<Row>& rows) {
  const int64_t T = 128, C = 512, LSLOTS = 8;
  std::vector<Unit> u;
  auto piece = [&](int64_t len, int64_t S, int band) {
    const int64_t nseg = (len + S - 1) / S;
    u.push_back(Unit{(int32_t)len, (int32_t)(nseg <= 1 ? len : S), (int16_t)std::max<int64_t>(nseg, 1), (int16_t)band});
  };
  for (const Row& r : rows) {
    if (r.len <= T) {
      u.push_back(Unit{(int32_t)r.len, (int32_t)r.len, 1, (int16_t)r.band});
    } else if (r.len <= C) {
      piece(r.len, std::max(seg_len_for(r.len), (r.len + LSLOTS - 1) / LSLOTS), r.band);
    } else {
      const int64_t S = std::max(seg_len_for(C), (C + LSLOTS - 1) / LSLOTS);
      for (int64_t b = 0; b < r.len; b += C) piece(std::min(C, r.len - b), S, r.band);
    }
  }
  return u;
}

// consecutive packing (the schedule the library has always built): units in order, <= 512 entries, <= 8 slots
Packing pack_consecutive(const std::vector<Unit>& u) {
  Packing p;
  p.tile_begin.push_back(0);
  int64_t nnz = 0, slots = 0, vrows = 0;
  for (size_t i = 0; i < u.size(); ++i) {
    const bool open = (int64_t)p.order.size() > p.tile_begin.back();
    const bool fits = nnz + u[i].len <= 512 && vrows + u[i].nseg <= 256 && (u[i].nseg <= 1 || slots + u[i].nseg <= 8);
    if (open && !fits) {
      p.tile_begin.push_back((int64_t)p.order.size());
      nnz = slots = vrows = 0;
    }
    p.order.push_back((int32_t)i);
    nnz += u[i].len, vrows += u[i].nseg;
    if (u[i].nseg > 1) slots += u[i].nseg;
  }
  if ((int64_t)p.order.size() > p.tile_begin.back()) p.tile_begin.push_back((int64_t)p.order.size());
  // longest first inside a tile, as the library lays a tile out
  for (int64_t t = 0; t + 1 < (int64_t)p.tile_begin.size(); ++t)
    std::stable_sort(p.order.begin() + p.tile_begin[(size_t)t], p.order.begin() + p.tile_begin[(size_t)t + 1],
                     [&](int32_t a, int32_t b) { return u[(size_t)a].len > u[(size_t)b].len; });
  return p;
}

// the limits the library packs with (idg_graph.hip: graph_build), with its environment switches
Limits library_limits() {
  Limits lim = idg_pack::dense_limits();
  if (const char* v = std::getenv("IDG_BALANCED_NNZ")) lim.tile_nnz = std::atoi(v);
  if (const char* v = std::getenv("IDG_BALANCED_ROUNDS")) lim.min_rounds = std::atoi(v);
  return lim;
}

double run_case(const std::string& name, const std::vector<Row>& rows, int groups, bool verbose, bool bound_tiles = false) {
  const std::vector<Unit> units = units_of(rows);
  int n_bands = 1;
  for (const Row& r : rows) n_bands = std::max(n_bands, r.band + 1);
  Limits lim = library_limits();
  lim.groups = groups;
  const int64_t tile_cap = lim.tile_nnz;
  CHECK(tile_cap <= 1024, "%s: a tile of %lld entries does not fit the kernel's LDS list", name.c_str(), (long long)tile_cap);
  Packing p, q;
  idg_pack::pack(units.data(), (int64_t)units.size(), n_bands, lim, &p);
  idg_pack::pack(units.data(), (int64_t)units.size(), n_bands, lim, &q);
  CHECK(p.order == q.order && p.tile_begin == q.tile_begin, "%s: two runs differ", name.c_str());
  CHECK(p.order.size() == units.size(), "%s: %zu units placed of %zu", name.c_str(), p.order.size(), units.size());
  CHECK(p.tile_begin.front() == 0 && p.tile_begin.back() == (int64_t)p.order.size(), "%s: offsets", name.c_str());
  std::vector<int> seen(units.size(), 0);
  for (int64_t t = 0; t < p.n_tiles(); ++t) {
    const int64_t b = p.tile_begin[(size_t)t], e = p.tile_begin[(size_t)t + 1];
    CHECK(e > b, "%s: tile %lld is empty", name.c_str(), (long long)t);
    int64_t nnz = 0, vrows = 0, slots = 0;
    std::vector<int32_t> vrow_unit;  // the tile's vrow list: the unit each vrow belongs to
    for (int64_t i = b; i < e; ++i) {
      const int32_t id = p.order[(size_t)i];
      CHECK(id >= 0 && (size_t)id < units.size(), "%s: unit id %d", name.c_str(), id);
      ++seen[(size_t)id];
      const Unit& u = units[(size_t)id];
      CHECK(u.band == units[(size_t)p.order[(size_t)b]].band, "%s: tile %lld mixes bands", name.c_str(), (long long)t);
      nnz += u.len, vrows += u.nseg;
      if (u.nseg > 1) slots += u.nseg;
      for (int s = 0; s < u.nseg; ++s) vrow_unit.push_back(id);
      if (i > b) {
        const Unit& w = units[(size_t)p.order[(size_t)i - 1]];
        CHECK(idg_pack::rounds_of(w.seg, lim.unroll) >= idg_pack::rounds_of(u.seg, lim.unroll),
              "%s: tile %lld is not longest first", name.c_str(), (long long)t);
      }
    }
    CHECK(nnz <= tile_cap, "%s: tile %lld holds %lld entries", name.c_str(), (long long)t, (long long)nnz);
    CHECK(vrows <= lim.tile_vrows, "%s: tile %lld holds %lld vrows", name.c_str(), (long long)t, (long long)vrows);
    CHECK(slots <= lim.lslots, "%s: tile %lld needs %lld slots", name.c_str(), (long long)t, (long long)slots);
    // a split row's segments are adjacent vrows of one tile
    for (size_t v = 0; v < vrow_unit.size();) {
      const Unit& u = units[(size_t)vrow_unit[v]];
      for (int s = 0; s < u.nseg; ++s)
        CHECK(v + (size_t)s < vrow_unit.size() && vrow_unit[v + (size_t)s] == vrow_unit[v], "%s: split row torn", name.c_str());
      v += (size_t)u.nseg;
    }
  }
  for (size_t i = 0; i < units.size(); ++i) CHECK(seen[i] == 1, "%s: unit %zu placed %d times", name.c_str(), i, seen[i]);
  const idg_pack::Stats s = idg_pack::stats_of(units.data(), p, lim);
  const double util = s.slots > 0 ? (double)s.rounds / (double)s.slots : 1.0;
  if (verbose) {
    const Packing c = pack_consecutive(units);
    const idg_pack::Stats cs = idg_pack::stats_of(units.data(), c, lim);
    std::printf("%s groups=%d units=%zu balanced: tiles=%lld rounds=%lld slots=%lld util=%.4f | consecutive: tiles=%lld util=%.4f\n",
                name.c_str(), groups, units.size(), (long long)s.tiles, (long long)s.rounds, (long long)s.slots, util,
                (long long)cs.tiles, cs.slots > 0 ? (double)cs.rounds / (double)cs.slots : 1.0);
    CHECK(cs.rounds == s.rounds, "%s: the two packings disagree on the work", name.c_str());
    if (bound_tiles) CHECK(s.tiles <= cs.tiles, "%s: %lld tiles, consecutive packing %lld", name.c_str(), (long long)s.tiles,
                            (long long)cs.tiles);
  }
  return util;
}

}  // namespace

int main(int argc, char** argv) {
  const int widths[] = {32, 16, 8, 4};
  {
    std::vector<Row> rows;
    const int64_t edge[] = {0, 1, 7, 8, 9, 63, 64, 65, 128, 129, 300, 512, 513, 1100};
    for (int band = 0; band < 2; ++band) {
      for (int64_t l : edge) rows.push_back(Row{l, band});
      for (int i = 0; i < 400; ++i) rows.push_back(Row{(int64_t)(i % 13), band});
    }
    for (int g : widths) run_case("edge-cases", rows, g, g == 16);
  }
  {
    std::vector<Row> rows(1000, Row{24, 0});
    for (int g : widths) run_case("all-equal", rows, g, g == 16);
    std::vector<Row> none;
    for (int g : widths) run_case("empty", none, g, false);
  }
  {
    std::vector<Row> rows(1, Row{100000, 0});
    for (int g : widths) run_case("giant-row", rows, g, g == 16);
  }
  {  // eight bands of mixed lengths
    std::vector<Row> rows;
    uint32_t x = 12345;
    for (int i = 0; i < 6000; ++i) {
      x = x * 1664525u + 1013904223u;
      const int64_t len = (x >> 8) % 97 == 0 ? 130 + (x >> 16) % 900 : (x >> 12) % 40;
      rows.push_back(Row{len, i * 8 / 6000});
    }
    for (int g : widths) run_case("eight-bands", rows, g, g == 16);
  }
  for (int a = 1; a + 1 < argc; a += 2) {
    std::FILE* f = std::fopen(argv[a], "r");
    CHECK(f != nullptr, "cannot open %s", argv[a]);
    long long n = 0;
    CHECK(std::fscanf(f, "%lld", &n) == 1 && n >= 0, "%s: bad header", argv[a]);
    std::vector<Row> rows((size_t)n);
    for (long long i = 0; i < n; ++i) {
      long long len = 0;
      int band = 0;
      CHECK(std::fscanf(f, "%lld %d", &len, &band) == 2 && len >= 0 && band >= 0 && band < 64, "%s: bad row %lld", argv[a], i);
      rows[(size_t)i] = Row{len, band};
    }
    std::fclose(f);
    const double min_util = std::atof(argv[a + 1]);
    for (int g : widths) {
      const double util = run_case(argv[a], rows, g, g == 16, g == 16);
      if (g == 16) CHECK(util >= min_util, "%s: utilisation %.4f below %.4f", argv[a], util, min_util);
    }
  }
  std::printf("ok\n");
  return 0;
}
