// Included by idg_score.hip inside its anonymous namespace (after the key helpers).
//
// ============================ bf16 bound scores for the threshold + collect form (round 5) =====================
// The exact kernels are bound by the fp32 matrix rate (64 cycles per v_mfma_f32_32x32x2_f32 and SIMD, and while one runs
// no other vector instruction of that SIMD does).  A bf16 MFMA does 8x the products in half the cycles.  Form 3
// (idg_score_collect.inc) only needs scores to DECIDE which few hundred items of a user get an exact score, so it runs on
// one-sided bounds of the exact fp32 score x(u, v):
//     s~(u, v)  = sum_k bf16(u_k) bf16(v_k)                         (fp32 accumulation on v_mfma_f32_32x32x16_bf16)
//     |s~ - x| <= c_d ||u|| ||v||,   c_d = bound_c(d)               (proof: DESIGN.md §4 "Top-K")
//     UB = s~ + cu(u) vb(v) >= x,    LB = s~ - cu(u) vb(v) <= x,    cu >= c_d ||u||, vb >= ||v||   (both bf16, rounded UP)
// and the bound term costs no vector instruction: it is one more feature — the tables carry a (d / 16 + 1)-th k-step whose
// only non-zero entry is vb(v) for an item and -cu(u) / +cu(u) for a user, so the MFMA chain itself delivers LB or UB.
// (Round 5 first ran the three-term split hi hi + hi lo + lo hi with a uniform 6e-5 ||u|| max||v|| margin — 24 MFMAs and
//  8 KiB of operands per wave and slab instead of 10 and 5 KiB: profiles/r05/topk_bf16_probe.txt, topk_form3.txt.)
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
// |s~ - x| / (||u|| ||v||): bf16 keeps 8 significant bits, so round-to-nearest moves either operand by at most 2^-8 relative
// and a product by at most 2^-7 (1 + 2^-9) = 0.0078278; the fp32 accumulation of the d + 1 products on either side adds at
// most d 2^-24 (the fmaf chain behind x) + (d + 16) 2^-23 (the matrix cores, whatever their order): 4.8e-5 at d = 256; the
// rounding of the bound product into the sum is in that.  Rounded up (tests/test_topk_bound_math.py checks the arithmetic).
__host__ __device__ inline float bound_c(int64_t d) { return 0.00786f + 2.0e-7f * (float)d; }

// The call's scalars (a few words of the workspace, zeroed by the first launch of every call)
enum : int {
  SC_VMAX = 0,             // max over the items of vb, as float bits (positive floats order as integers)
  SC_REDO = 1,             // users the finish could not serve and handed to topk_redo_kernel
  SC_THRESHOLD = 2,        // more of those than this: the call is answered by the exact form as a whole (SC_NEVER: never)
  SC_ITEMS_IRREGULAR = 3,  // an item row holds a NaN / an infinity / a norm beyond ROW_NORM_MAX: likewise
  COLLECT_SCALARS = 4
};
constexpr uint32_t SC_NEVER = 0xFFFFFFFFu;
// (after the finish) does the exact form answer this call?  What the redo and the gated exact launches all evaluate.
__device__ __forceinline__ bool fallback_taken(const uint32_t* __restrict__ scalars) {
  const uint32_t thr = scalars[SC_THRESHOLD];
  return thr != SC_NEVER && (scalars[SC_ITEMS_IRREGULAR] != 0u || scalars[SC_REDO] > thr);
}

__device__ __forceinline__ __bf16 bf16_round_up(float x) {  // the smallest bf16 >= x (x >= 0)
  const uint32_t b = (__float_as_uint(x) + 0xFFFFu) & 0xFFFF0000u;
  return (__bf16)__uint_as_float(b);  // (exact: the low 16 bits are zero)
}

// An upper bound of a row's Euclidean norm from its 8-feature pieces (`groups` lanes per row, a power of two), taken so
// that nothing on the way under- or overflows (VERDICT r05: with sqrt(sum v^2) a row whose elements lie below ~1e-23 got
// the bound 0 while bf16's operand error stays relative): the squares are those of the row scaled by a power of two
// (exact) that brings its largest element into [0.5, 1), the root is scaled back.  fp32 rounding of the sum (8 chained
// fmaf + a tree of log2(groups) adds), of the root and of the products below: under 1e-6 relative — covered by 1.000004.
// *regular = the row can take part in the bound arithmetic: every element finite and the norm at most ROW_NORM_MAX
// (a NaN fails every comparison); the callers zero an irregular row's operands and route it to an exact path.
// The result is at least ROW_NORM_MIN: products of operands this small leave fp32's normal range, where the matrix
// cores may flush — an absolute error of at most (d + 1) 2^-126 per score, which c_d 2^-80 covers many times over.
constexpr float ROW_NORM_MIN = 0x1p-40f, ROW_NORM_MAX = 0x1p60f;
__device__ __forceinline__ float row_norm_up(const float (&v)[8], const int groups, bool* regular) {
  float mx = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) mx = fmaxf(mx, fabsf(v[e]));
  for (int o = 1; o < groups; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, WAVE));
  int ex = 0;
  (void)frexpf(mx, &ex);  // mx = m 2^ex, m in [0.5, 1); 0 -> 0 (infinities and NaNs: the sum below carries them)
  float sq = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float sv = ldexpf(v[e], -ex);
    sq = __builtin_fmaf(sv, sv, sq);
  }
  for (int o = 1; o < groups; o <<= 1) sq += __shfl_xor(sq, o, WAVE);
  const float nr = ldexpf(sqrtf(sq) * 1.000004f, ex);
  *regular = nr <= ROW_NORM_MAX;
  return fmaxf(nr, ROW_NORM_MIN);  // (fmaxf drops a NaN: *regular was taken first)
}

// Rows of an fp32 table (d = 16 KS, KS = 4 / 8 / 16) as bf16 with the bound k-step appended, 16 bytes (8 features) per
// thread.  bound[row] = the row's bound factor as a float (items: vb; users: cu); *max_bound_bits (nullable) = max over
// rows (positive floats order as integers).  rows_idx (nullable): gather row rows_idx[r] instead of r (the batch's users).
//   tiled = 0 (users): row-major, KS + 2 k-step groups of 32 bytes per row: group k < KS = features [16 k, 16 k + 16) (the 8
//       of half h = 0, then the 8 of h = 1); group KS = [-cu, 0 x 15] (-> LB), group KS + 1 = [+cu, 0 x 15] (-> UB).
//   tiled = 1 (items): tiles of 32 rows, KS + 1 blocks of 1 KiB each; inside block k lane (i, h) = i + 32 h holds row i's
//       features [16 k + 8 h, + 8) — so one wave-wide 16-byte load of a producer is ONE contiguous KiB = 8 cache lines
//       instead of 64 (one per lane): the CU's address path, not the matrix pipe, is what such loads cost; block KS holds
//       [vb, 0 x 7] for lane (i, 0), zeros for lane (i, 1).  Rows up to the next multiple of 32 are written as zeros.
__global__ __launch_bounds__(BLOCK) void bound_table_kernel(const float* __restrict__ X, const int64_t* __restrict__ rows_idx,
                                                            int64_t n_rows, int64_t n_rows_padded, int64_t d, int log2_groups,
                                                            int tiled, float c, __bf16* __restrict__ out, float* __restrict__ bound,
                                                            uint32_t* __restrict__ max_bound_bits, uint32_t* __restrict__ zero_scalars,
                                                            uint32_t fallback_threshold) {
  __shared__ float s_max[BLOCK / WAVE];
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  // (the users' launch, which runs first, resets the call's scalars for the items' launch and everything behind it)
  if (zero_scalars && t < COLLECT_SCALARS) zero_scalars[t] = t == SC_THRESHOLD ? fallback_threshold : 0u;
  const int G = 1 << log2_groups, KS = G >> 1;
  const int64_t r = t >> log2_groups;
  const int g = (int)(t & (G - 1));
  const bool live = r < n_rows;
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (live) {
    const float* x = X + (rows_idx ? rows_idx[r] : r) * d + 8 * g;
    const float4 a = *reinterpret_cast<const float4*>(x), b = *reinterpret_cast<const float4*>(x + 4);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
  }
  // an upper bound of the norm, as a bf16; users: times c.  An IRREGULAR row (a NaN, an infinity, a norm beyond 2^60) gets
  // zero operands and the bound +inf: the finish hands such a user to the exact pass over the whole catalogue
  bool regular;
  const float nr = row_norm_up(v, G, &regular);
  regular = regular || !live;
  bf16x8 hi;
#pragma unroll
  for (int e = 0; e < 8; ++e) hi[e] = (__bf16)(regular ? v[e] : 0.f);
  const __bf16 bb = !live || !regular ? (__bf16)0.f : bf16_round_up(tiled ? nr : c * nr);
  if (r < n_rows_padded) {
    bf16x8 zero, first;
#pragma unroll
    for (int e = 0; e < 8; ++e) zero[e] = (__bf16)0.f, first[e] = (__bf16)0.f;
    first[0] = bb;
    const int k = g >> 1, h = g & 1;
    if (tiled) {
      char* tile = reinterpret_cast<char*>(out) + (r >> 5) * ((int64_t)(KS + 1) * 1024) + ((int)(r & 31) + 32 * h) * 16;
      *reinterpret_cast<bf16x8*>(tile + k * 1024) = hi;
      if (g < 2) *reinterpret_cast<bf16x8*>(tile + KS * 1024) = g == 0 ? first : zero;
    } else {
      char* row = reinterpret_cast<char*>(out) + r * ((int64_t)(KS + 2) * 32);
      *reinterpret_cast<bf16x8*>(row + k * 32 + h * 16) = hi;
      if (g == 0) {
        bf16x8 neg = first;
        neg[0] = -bb;
        *reinterpret_cast<bf16x8*>(row + KS * 32) = neg;
        *reinterpret_cast<bf16x8*>(row + (KS + 1) * 32) = first;
      } else if (g == 1) {
        *reinterpret_cast<bf16x8*>(row + KS * 32 + 16) = zero;
        *reinterpret_cast<bf16x8*>(row + (KS + 1) * 32 + 16) = zero;
      }
    }
  }
  if (live && g == 0) bound[r] = regular ? (float)bb : __builtin_inff();
  if (max_bound_bits) {  // one atomic per workgroup (tens of thousands of atomics on one word serialise)
    float m = (float)bb;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, WAVE));
    if (threadIdx.x % WAVE == 0) s_max[threadIdx.x / WAVE] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < BLOCK / WAVE; ++w) m = fmaxf(m, s_max[w]);
      atomicMax(max_bound_bits, __float_as_uint(m));
    }
  }
}

// The items' (tiled) table through LDS: one workgroup per tile of 32 rows, 32 x d / 8 threads.  Reads run along the rows (a
// wave covers whole rows: 2 KiB contiguous per instruction), the tile image is put together in LDS, and it leaves as
// contiguous 16-byte pieces — bound_table_kernel's tiled stores were 16 bytes per lane into d / 8 different KiB blocks
// (17 us for 38,048 x 64, 3.6 ms for 5 M x 256: a third of a 1024-user call at that geometry).
template <int KS>
__global__ __launch_bounds__(64 * KS) void item_table_kernel(const float* __restrict__ X, int64_t n_rows, __bf16* __restrict__ out,
                                                            float* __restrict__ bound, uint32_t* __restrict__ scalars) {
  constexpr int G = 2 * KS, NT = 64 * KS, D = 16 * KS;
  __shared__ bf16x8 s_tile[(KS + 1) * 64];
  __shared__ float s_max[NT / WAVE];
  const int tid = threadIdx.x, r_in = tid / G, g = tid % G;
  const int64_t r = (int64_t)blockIdx.x * 32 + r_in;
  const bool live = r < n_rows;
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (live) {
    const float* x = X + r * D + 8 * g;
    const float4 a = *reinterpret_cast<const float4*>(x), b = *reinterpret_cast<const float4*>(x + 4);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
  }
  // (as bound_table_kernel: an upper bound of the norm.)  An IRREGULAR item row — a NaN, an infinity, a norm beyond 2^60 —
  // touches every user's ranking: it is flagged (scalars[SC_ITEMS_IRREGULAR]) and the call as a whole is answered by the
  // exact form (fallback_taken); its operands here are zeros so that the passes that still run stay finite
  bool regular;
  const float nr = row_norm_up(v, G, &regular);
  regular = regular || !live;
  bf16x8 hi, zero;
#pragma unroll
  for (int e = 0; e < 8; ++e) hi[e] = (__bf16)(regular ? v[e] : 0.f), zero[e] = (__bf16)0.f;
  const __bf16 bb = !live || !regular ? (__bf16)0.f : bf16_round_up(nr);
  if (!regular && g == 0) atomicOr(scalars + SC_ITEMS_IRREGULAR, 1u);
  s_tile[(g >> 1) * 64 + r_in + 32 * (g & 1)] = hi;
  if (g < 2) {
    bf16x8 first = zero;
    first[0] = bb;
    s_tile[KS * 64 + r_in + 32 * g] = g == 0 ? first : zero;
  }
  if (live && g == 0) bound[r] = (float)bb;
  float m = (float)bb;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, WAVE));
  if (tid % WAVE == 0) s_max[tid / WAVE] = m;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < NT / WAVE; ++w) m = fmaxf(m, s_max[w]);
    atomicMax(scalars + SC_VMAX, __float_as_uint(m));
  }
  bf16x8* dst = reinterpret_cast<bf16x8*>(reinterpret_cast<char*>(out) + (int64_t)blockIdx.x * ((KS + 1) * 1024));
  for (int e = tid; e < (KS + 1) * 64; e += NT) dst[e] = s_tile[e];
}

// The producer half on the bound tables, KS = d / 16 data k-steps + the bound k-step (UB: + cu vb, else - cu vb): wave `wave`
// (0..3) scores items 32 wave .. 32 wave + 31 of every slab it walks (slab t of the walk = slab t * slab_stride of the
// chunk) for the block's 64 users into s_buf[t & 1] and meets the consumers at barrier t.  The consumers open with one
// extra barrier (see IDG_ITER).
// User operands: in registers up to d = 128 (2 x 9 x 4 of them); at d = 256 (KS = 16) they come from the workgroup's LDS copy
// s_users — entry ((2 k + h) 64 + user) of 16 bytes = user's features [16 k + 8 h, + 8), k = KS the bound k-step of this
// pass (filled by the kernel before the roles split: a wave's 16-byte reads of one (k, h) are then conflict-free).
template <int KS, bool UB>
__device__ __forceinline__ void bound_produce(const __bf16* __restrict__ Us, const __bf16* __restrict__ Vs, int64_t Bt, int64_t I,
                                              const int64_t b0, const int64_t c_lo, const int wave, const int lane, const int n_slabs,
                                              const int slab_stride, float (*s_buf)[FT_USERS * FT_LD], const bf16x8* s_users) {
  constexpr int KS1 = KS + 1;
  constexpr bool ULDS = KS > 8;
  constexpr int UREG = ULDS ? 1 : KS1;
  if (n_slabs <= 0) {
    __syncthreads();  // the consumers' opening barrier
    return;
  }
  const int i = lane & 31, h = lane >> 5;
  const int64_t bu0 = b0 + i < Bt ? b0 + i : Bt - 1;
  const int64_t bu1 = b0 + 32 + i < Bt ? b0 + 32 + i : Bt - 1;
  const char* u0 = reinterpret_cast<const char*>(Us) + bu0 * ((KS + 2) * 32) + h * 16;
  const char* u1 = reinterpret_cast<const char*>(Us) + bu1 * ((KS + 2) * 32) + h * 16;
  bf16x8 ua0[UREG], ua1[UREG];
#pragma unroll
  for (int k = 0; k < UREG; ++k) {
    const int grp = k < KS ? k : (UB ? KS + 1 : KS);
    ua0[k] = *reinterpret_cast<const bf16x8*>(u0 + grp * 32);
    ua1[k] = *reinterpret_cast<const bf16x8*>(u1 + grp * 32);
  }
  const bf16x8* su0 = s_users + 64 * h + i;  // (ULDS) + 128 k: k-step k of users i / 32 + i
  // the item table is TILED (bound_table_kernel): this wave's column tile of slab t is tile (c_lo + 32 wave) / 32 + 4 t stride,
  // and lane L reads 16 bytes at L * 16 of each of the tile's KS + 1 one-KiB blocks — a contiguous KiB per wave-wide load
  const int64_t tile0 = (c_lo + 32 * wave) / 32, last_tile = (I - 1) / 32;
  auto item_row = [&](int t) {
    int64_t tl = tile0 + (int64_t)t * slab_stride * (FT_SLAB / 32);
    tl = tl < last_tile ? tl : last_tile;  // (past the catalogue: a valid tile nobody's scores are read from)
    return reinterpret_cast<const char*>(Vs) + tl * (KS1 * 1024) + lane * 16;
  };
  // One producer wave per SIMD has nobody to hide behind, so the wave's own instruction stream is software-pipelined:
  //   * item operands travel TWO slabs ahead of the MFMAs that use them, in two register sets that are refilled IN PLACE — as
  //     soon as the two MFMAs of k-step k of slab t have issued, the register they read takes the same k-step of slab t + 2.
  //     Loads are issued and waited for by hand (asm; left to the compiler each load lands right before its MFMAs); in issue
  //     order the loads younger than (slab t, k-step k) are always 2 KS1 - 1, hence the constant in the wait;
  //   * the 32 LDS stores of slab t - 1 are issued BETWEEN the MFMAs of slab t, spread over its k-steps, from a second pair
  //     of accumulators: the matrix pipe does not idle while a slab is written out and the barrier is met.
  // Barrier T (slab T complete in s_buf[T & 1]) follows the iteration that stored slab T.
  typedef float f32x4_ __attribute__((ext_vector_type(4)));
  f32x4_ qa[KS1], qb[KS1];
  // block K of the tile at `ptr` (the instruction's offset field ends at 4095: blocks 4 .. 7 go through ptr + 4096, ...)
#define IDG_LD1(QK, K, ptr)                                                                                          \
  {                                                                                                                  \
    const char* p_ = (ptr) + ((K) >> 2) * 4096;                                                                      \
    switch ((K) & 3) {                                                                                               \
      case 0: asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(QK) : "v"(p_)); break;               \
      case 1: asm volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=&v"(QK) : "v"(p_)); break;   \
      case 2: asm volatile("global_load_dwordx4 %0, %1, off offset:2048" : "=&v"(QK) : "v"(p_)); break;   \
      default: asm volatile("global_load_dwordx4 %0, %1, off offset:3072" : "=&v"(QK) : "v"(p_)); break;  \
    }                                                                                                                \
  }
#define IDG_WAITK(QK)                                                                                                \
  {                                                                                                                  \
    if (KS1 == 5) asm volatile("s_waitcnt vmcnt(9)" : "+v"(QK));                                        \
    else if (KS1 == 9) asm volatile("s_waitcnt vmcnt(17)" : "+v"(QK));                                  \
    else asm volatile("s_waitcnt vmcnt(33)" : "+v"(QK));                                                \
  }
  // iteration T: the MFMAs of slab T into (A0, A1) from register set Q — refilled for slab T + 2 —, the stores of slab T - 1
  // from (P0, P1), barrier T - 1.  EVERY iteration is the same code: iteration 0 stores zeros as "slab -1" into buffer 1
  // (which nobody reads before slab 1 is in it) and meets the consumers' opening barrier — a first iteration without stores
  // would be peeled off by the compiler, and every merge of control flow it creates is a place for register copies (below).
#define IDG_ITER(Q, T, A0, A1, P0, P1)                                                                               \
  {                                                                                                                  \
    float* s_prev = s_buf[((T) - 1) & 1];                                                                            \
    const char* next_ = item_row((T) + 2);                                                                           \
    bf16x8 an0_ = ua0[0], an1_ = ua1[0];                                                                             \
    if (ULDS) an0_ = su0[0], an1_ = su0[32];                                                                         \
    _Pragma("unroll") for (int k = 0; k < KS1; ++k) {                                                                \
      const bf16x8 a0_ = ULDS ? an0_ : ua0[ULDS ? 0 : k], a1_ = ULDS ? an1_ : ua1[ULDS ? 0 : k];                     \
      if (ULDS && k + 1 < KS1) an0_ = su0[128 * (k + 1)], an1_ = su0[128 * (k + 1) + 32]; /* one k-step ahead */     \
      IDG_WAITK(Q[k]);                                                                                               \
      const bf16x8 bk = __builtin_bit_cast(bf16x8, Q[k]);                                                            \
      A0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0_, bk, k == 0 ? zero16 : A0, 0, 0, 0);                          \
      A1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1_, bk, k == 0 ? zero16 : A1, 0, 0, 0);                          \
      _Pragma("unroll") for (int r = (16 * k) / KS1; r < (16 * (k + 1)) / KS1; ++r) {                                \
        const int row = idg::mfma_c_row(r, h);                                                              \
        s_prev[row * FT_LD + 32 * wave + i] = P0[r];                                                                 \
        s_prev[(32 + row) * FT_LD + 32 * wave + i] = P1[r];                                                          \
      }                                                                                                              \
      IDG_LD1(Q[k], k, next_);                                                                                       \
    }                                                                                                                \
    __syncthreads(); /* barrier T - 1 (T = 0: the opening barrier) */                                                \
  }
  f32x16 zero16;
#pragma unroll
  for (int r = 0; r < 16; ++r) zero16[r] = 0.f;
  f32x16 xa0 = zero16, xa1 = zero16, xb0 = zero16, xb1 = zero16;
  {
    const char* r0 = item_row(0);
    const char* r1 = item_row(1);
#pragma unroll
    for (int k = 0; k < KS1; ++k) IDG_LD1(qa[k], k, r0);
#pragma unroll
    for (int k = 0; k < KS1; ++k) IDG_LD1(qb[k], k, r1);
  }
  // Everything issued so far must have ARRIVED on every path into the loop.  (1) The compiler waits for its own loads — the
  // user operands — where they are first used, counting only its own: left inside the loop, those waits would drain the
  // hand-issued item loads in every iteration; this asm reads all of them, once, here.  (2) The in-flight item registers
  // are asm outputs the compiler believes to be ready, and wherever control flow merges between a load and its use it may
  // COPY them — a copy of a register whose load has not landed copies garbage (seen with a `break` between the two halves
  // of the body, and with a last odd slab handled after the loop).  At the loop entry the copies are harmless after this
  // wait; the body is one straight pair of iterations; nothing reads the registers after it.
#pragma unroll
  for (int k = 0; k < UREG; ++k) asm volatile("" : "+v"(ua0[k]), "+v"(ua1[k]));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // An odd slab count runs one phantom slab (clamped loads, MFMAs nobody stores) in the second half of its last pair.
  // n_slabs >= 1 here: the loop runs at least once, nothing merges behind it.
  for (int t = 0; t < n_slabs; t += 2) {
    IDG_ITER(qa, t, xa0, xa1, xb0, xb1);
    IDG_ITER(qb, t + 1, xb0, xb1, xa0, xa1);  // (t + 1 == n_slabs: stores slab n_slabs - 1, meets the last barrier)
  }
  // The last MFMAs may be only a barrier (passed at once by the last wave to arrive) away from the first read of their
  // accumulators, and the wait states the compiler puts between them were seen to be too few on this chip (a register copy
  // 11 wait states behind a pair of v_mfma_f32_32x32x16_bf16 read one accumulator register before it was written: 1 user in
  // 1,000 lost an item of a chunk's last slab).  Whatever reads them next comes after this.
  asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" : "+v"(xa0), "+v"(xa1), "+v"(xb0), "+v"(xb1));
  if (!(n_slabs & 1)) {  // the last slab of an even count is still in its accumulators
    float* s_last = s_buf[(n_slabs - 1) & 1];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = idg::mfma_c_row(r, h);
      s_last[row * FT_LD + 32 * wave + i] = xb0[r];
      s_last[(32 + row) * FT_LD + 32 * wave + i] = xb1[r];
    }
    __syncthreads();  // barrier n_slabs - 1
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#undef IDG_LD1
#undef IDG_WAITK
#undef IDG_ITER
}

// The same producer for TWO workgroups per CU (d = 64): at most 128 registers — one accumulator pair, one item register set
// refilled in place ONE slab ahead — and no software pipelining of its own: while this wave writes a slab out and waits at
// the barrier, the other workgroup's producer on the same SIMD has the matrix pipe, and the two consumer waves per SIMD
// interleave their vector work.
template <int KS, bool UB>
__device__ __forceinline__ void bound_produce_lean(const __bf16* __restrict__ Us, const __bf16* __restrict__ Vs, int64_t Bt, int64_t I,
                                                   const int64_t b0, const int64_t c_lo, const int wave, const int lane,
                                                   const int n_slabs, const int slab_stride, float (*s_buf)[FT_USERS * FT_LD]) {
  constexpr int KS1 = KS + 1;
  __syncthreads();  // the consumers' opening barrier
  if (n_slabs <= 0) return;
  const int i = lane & 31, h = lane >> 5;
  const int64_t bu0 = b0 + i < Bt ? b0 + i : Bt - 1;
  const int64_t bu1 = b0 + 32 + i < Bt ? b0 + 32 + i : Bt - 1;
  const char* u0 = reinterpret_cast<const char*>(Us) + bu0 * ((KS + 2) * 32) + h * 16;
  const char* u1 = reinterpret_cast<const char*>(Us) + bu1 * ((KS + 2) * 32) + h * 16;
  bf16x8 ua0[KS1], ua1[KS1];
#pragma unroll
  for (int k = 0; k < KS1; ++k) {
    const int grp = k < KS ? k : (UB ? KS + 1 : KS);
    ua0[k] = *reinterpret_cast<const bf16x8*>(u0 + grp * 32);
    ua1[k] = *reinterpret_cast<const bf16x8*>(u1 + grp * 32);
  }
  const int64_t tile0 = (c_lo + 32 * wave) / 32, last_tile = (I - 1) / 32;
  auto item_row = [&](int t) {
    int64_t tl = tile0 + (int64_t)t * slab_stride * (FT_SLAB / 32);
    tl = tl < last_tile ? tl : last_tile;
    return reinterpret_cast<const char*>(Vs) + tl * (KS1 * 1024) + lane * 16;
  };
  typedef float f32x4_ __attribute__((ext_vector_type(4)));
  f32x4_ q[KS1];
#define IDG_LD1(QK, K, ptr)                                                                                          \
  {                                                                                                                  \
    const char* p_ = (ptr) + ((K) >> 2) * 4096;                                                                      \
    switch ((K) & 3) {                                                                                               \
      case 0: asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(QK) : "v"(p_)); break;                          \
      case 1: asm volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=&v"(QK) : "v"(p_)); break;              \
      case 2: asm volatile("global_load_dwordx4 %0, %1, off offset:2048" : "=&v"(QK) : "v"(p_)); break;              \
      default: asm volatile("global_load_dwordx4 %0, %1, off offset:3072" : "=&v"(QK) : "v"(p_)); break;             \
    }                                                                                                                \
  }
  {
    const char* r0 = item_row(0);
#pragma unroll
    for (int k = 0; k < KS1; ++k) IDG_LD1(q[k], k, r0);
  }
  // (as in bound_produce: the user operands and the first loads have ARRIVED on every path into the loop)
#pragma unroll
  for (int k = 0; k < KS1; ++k) asm volatile("" : "+v"(ua0[k]), "+v"(ua1[k]));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  f32x16 zero16;
#pragma unroll
  for (int r = 0; r < 16; ++r) zero16[r] = 0.f;
  for (int t = 0; t < n_slabs; ++t) {
    const char* next_ = item_row(t + 1);
    f32x16 a0 = zero16, a1 = zero16;
#pragma unroll
    for (int k = 0; k < KS1; ++k) {
      // in issue order the loads younger than (slab t, k-step k) are always KS1 - 1 = 4
      asm volatile("s_waitcnt vmcnt(4)" : "+v"(q[k]));
      static_assert(KS1 == 5, "the wait above is written for d = 64");
      const bf16x8 bk = __builtin_bit_cast(bf16x8, q[k]);
      a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ua0[k], bk, a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ua1[k], bk, a1, 0, 0, 0);
      IDG_LD1(q[k], k, next_);
    }
    // (explicit wait states between the last MFMAs and the first read of their accumulators: bound_produce)
    asm volatile("s_nop 15\n\ts_nop 7" : "+v"(a0), "+v"(a1));
    float* s_score = s_buf[t & 1];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = idg::mfma_c_row(r, h);
      s_score[row * FT_LD + 32 * wave + i] = a0[r];
      s_score[(32 + row) * FT_LD + 32 * wave + i] = a1[r];
    }
    __syncthreads();  // barrier t
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#undef IDG_LD1
}
