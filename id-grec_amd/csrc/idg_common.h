// Shared internals of libidgrec.so: error reporting, HIP call checking and the host-side size arithmetic.
// (Device-side helpers: idg_device.h, for .hip files only.)
#pragma once
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "idgrec.h"

namespace idg {

// Thread-local "last error" string behind idg_last_error().
void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
const char* get_error();

inline int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  set_error("%s", buf);
  return code;
}

// Workspace sub-buffers start at multiples of 256 bytes; padded operands are rounded up to whole tiles.
inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }
inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// ---- The aliasing checks of the entry points: which bytes a call reads or writes, and whether two such ranges meet.
struct Span {
  const void* ptr;
  size_t bytes;
};

// [p, p + bytes) and [q, q + bytes2) share a byte (an absent or empty range shares none)
inline bool overlap(const void* p, size_t bytes, const void* q, size_t bytes2) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return p && q && bytes && bytes2 && a < b + bytes2 && b < a + bytes;
}

// bytes from the first to one past the last float of an [n, d] panel read or written with leading dimension ld
inline size_t extent(int64_t n, int64_t d, int64_t ld) { return ((size_t)(n - 1) * (size_t)ld + (size_t)d) * sizeof(float); }

// does any of these outputs overlap any of these inputs / do any two of these outputs overlap
inline bool outputs_meet_inputs(const Span* outs, int n_out, const Span* ins, int n_in) {
  for (int o = 0; o < n_out; ++o)
    for (int q = 0; q < n_in; ++q)
      if (overlap(outs[o].ptr, outs[o].bytes, ins[q].ptr, ins[q].bytes)) return true;
  return false;
}
inline bool outputs_meet(const Span* outs, int n_out) {
  for (int o = 0; o < n_out; ++o)
    for (int q = o + 1; q < n_out; ++q)
      if (overlap(outs[o].ptr, outs[o].bytes, outs[q].ptr, outs[q].bytes)) return true;
  return false;
}

// out[e] (+)= the sum over s of part[s * count + e], e < count, in ONE published order: lane group g of 16 adds the slices
// g, g + 16, g + 32, ... ascending, then the 16 group sums are added g = 0 .. 15 (wgrad_reduce_kernel, idg_dense.hip: the
// only slice reduction of the library).  `part` holds [slices][count] floats.
int slices_reduce(const float* part, int64_t slices, int64_t count, float* out, bool accumulate, void* stream);

// A row bitmap is about to be rewritten by a library call: live-unit lists registered for it (idg_graph_live_units)
// describe its old contents and are dropped (idg_graph.hip).  bytes: extent of the write when the caller knows it (lists
// registered for a sub-range starting inside it go too); 0 = lists registered at `bitmap` itself.
void rows_changed(const void* bitmap, size_t bytes = 0);

// Library-internal forms of two entry points, for idg_step.cpp's one-call step (fewer launches per step on the host):
// idg_bpr_plan_rows_f32 whose first kernel also zeroes two words (`zero2`, nullable: the header of the unit list about to
// be built) and which may sort up to 4096 pairs with ONE workgroup (`one_launch_sort`: a launch less where the side stream
// has slack); idg_graph_live_units without its own clearing of that header.
int bpr_plan_rows(const int64_t* users, const int64_t* pos, const int64_t* neg, int64_t B, int64_t num_users, int64_t n, void* ws,
                  uint32_t* bitmap, uint32_t* zero2, bool one_launch_sort, void* stream);
// The sorted (row, slot) lists of a plan idg_bpr_plan_f32 left in a BPR workspace of batch size B (idg_au.hip scatters
// through the plan of (users, pos, pos)).
void bpr_plan_lists(const void* ws, int64_t B, const int32_t** skeys, const int32_t** sslots);
int live_units_prezeroed(const idg_graph* g, const uint32_t* bitmap, void* units_ws, int64_t max_rows, void* stream);

}  // namespace idg

#define IDG_REQUIRE(cond, ...)                                   \
  do {                                                           \
    if (!(cond)) return idg::fail(IDG_E_INVALID, __VA_ARGS__);   \
  } while (0)

#define IDG_HIP(call)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return idg::fail(e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice ? IDG_E_NODEVICE \
                                                                             : IDG_E_HIP,  \
                       "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__,    \
                       __LINE__);                                                          \
  } while (0)
