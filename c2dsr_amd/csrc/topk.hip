// Full-catalogue top-K recommendation and full ranking: for query rows q [M][d] and one classifier head W [n][d],
// b [n], the scores s(i, j) = q_i · W_j + b_j over ALL j ∈ [0, n) are swept once and never written to memory; per row
// the sweep keeps the k best (score, id) pairs and counts the columns that beat the row's target.
//
// Data path: the S phase of the fused CE forward (ce3.hip MODE 0) — split-bf16 operand images [rows][2·D] "hi ‖ lo",
// every product as three v_mfma_f32_16x16x32_bf16 (hi·hi + lo·hi + hi·lo, fp32 accumulate), stationary = 128 query
// rows per workgroup (4 waves × two 16-row blocks, their hi / lo k-slices in registers), swept = 32-row W tiles
// through two LDS buffers (register-staged: tile t+1's global loads are issued before the products of tile t and
// stored to LDS after them; one barrier per tile).  There is no second product, so the MFMAs are compiler-visible
// builtins and the epilogue is plain C++.
//
// One instruction sequence per score: an element of S is the chain over ks = 0 .. D/32-1 of the three MFMAs, then
// one fp32 add of b_j.  It depends on the element's own operand rows only — not on the tile, the position in the
// tile or the column split that holds it.  The target's score comes out of the same routine: before the sweep the
// workgroup runs it on four gathered tiles whose swept rows are its own rows' target rows and reads the diagonal.
//
// Selection: a (score, id) pair is one 64-bit key, larger = better (order-preserving map of the fp32 bits in the high
// word, ~id in the low word: score descending, id ascending among bit-equal scores).  Every row has a candidate list
// of CAP = 2·KP keys in the workspace (KP = k rounded up to 32 / 64 / 128; the lists of a workgroup stay L2-resident),
// an LDS fill count and an LDS threshold (the k-th best score so far, −inf at first).  A column whose score is
// strictly above the threshold (columns arrive by ascending id, so an equal later score loses the tie) and that is not
// excluded is appended with an LDS integer atomic.  A row's list is compacted — sorted by counting, for each key,
// the keys above it; the k best written back in order — once fewer than 32 slots (one tile's worth) are free, which
// also raises the threshold.  A row's candidates are produced by one wave only, so appends, compaction and the
// threshold need no workgroup barrier.  The final list is a pure function of the candidate SET, and the merge kernel
// takes the k best of the union of the splits' lists: results do not depend on n_split or on scheduling.
#include "img.h"

namespace {

using namespace c2img;

typedef unsigned long long u64;

constexpr int TK_T = 32;        // swept rows per LDS tile
constexpr int TK_RB = 128;      // stationary rows per workgroup
constexpr int TK_KMAX = 128;    // largest k
constexpr int TK_CAPMAX = 2 * TK_KMAX;

inline int tk_kp(int k) {
  int p = 32;
  while (p < k) p <<= 1;
  return p;
}
// keys per candidate list (64 / 128 / 256).  Measured at the benchmark head shapes (tools/topk_micro.py, k = 20):
// lists of 4·KP keys — fewer, larger compactions — with a merge that took several lists per round ran 1.66× slower
// (2407 vs 1448 µs, Movie-Book head b): the counting sort's cost grows with the square of the list
inline int tk_cap(int k) { return 2 * tk_kp(k); }

__device__ __forceinline__ u64 tk_key(float s, int id) {
  unsigned u = __float_as_uint(s);
  u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
  return ((u64)u << 32) | (unsigned)(~id);
}
__device__ __forceinline__ float tk_score(u64 key) {
  unsigned u = (unsigned)(key >> 32);
  u ^= (u >> 31) ? 0x80000000u : 0xffffffffu;
  return __uint_as_float(u);
}
__device__ __forceinline__ int tk_id(u64 key) { return (int)~(unsigned)key; }

// LDS traffic between the lanes of one wave (in-order LDS queue; the fences keep the compiler from moving accesses)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One wave: the list L[0 .. c) (distinct keys, c <= TK_CAPMAX) → its min(c, k) largest keys in descending order, in
// place.  S: TK_CAPMAX + 1 keys of LDS scratch private to the wave; S[TK_CAPMAX] receives the k-th key when c >= k.
__device__ __forceinline__ void tk_compact(u64* __restrict__ L, int c, int k, u64* S, int lane) {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // the other lanes' appends
  for (int e = lane; e < c; e += 64) S[e] = L[e];
  wave_sync();
  for (int e = lane; e < c; e += 64) {
    const u64 me = S[e];
    int r = 0;
    for (int f = 0; f < c; ++f) r += S[f] > me ? 1 : 0;
    if (r < k) L[r] = me;
    if (r == k - 1) S[TK_CAPMAX] = me;
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  wave_sync();
}

#define TK_MF(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0)

// grid: (row block, column split) pairs, split-major, dealt to the XCDs in contiguous ranges (ce3.hip's map)
template <int D>
__global__ __launch_bounds__(256, 1) void topk_sweep_kernel(
    const bf16* __restrict__ Qx, const bf16* __restrict__ Wx, const float* __restrict__ bias, int M, int n, int k,
    int cap, int per_split, const int64_t* __restrict__ target, const int64_t* __restrict__ exclude, int E,
    const int64_t* __restrict__ dom, int which, const int* __restrict__ bad, u64* __restrict__ lists,
    int* __restrict__ pcnt, int* __restrict__ rcnt, int mpad) {
  constexpr int D2 = 2 * D;           // image columns (hi ‖ lo)
  constexpr int ROWB = D2 * 2;        // bytes per image row
  constexpr int CPR = ROWB / 16;      // 16-byte chunks per row (a multiple of 16)
  constexpr int KS = D / 32;          // k-steps
  constexpr int NLD = TK_T * CPR / 256;  // 16-byte loads per thread per tile
  __shared__ __attribute__((aligned(16))) char img[2][TK_T * ROWB];
  __shared__ __attribute__((aligned(16))) float bt[2][TK_T];
  __shared__ int cnt[TK_RB];
  __shared__ float thr[TK_RB];
  __shared__ int tg[TK_RB];
  __shared__ int act[TK_RB];
  __shared__ u64 scr[4][TK_CAPMAX + 1];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l16 = lane & 15, g = lane >> 4;
  const int nrb = mpad / TK_RB, nb = (int)gridDim.x;
  const int pidx = nb % 8 == 0 ? (int)(blockIdx.x & 7) * (nb >> 3) + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  const int split = pidx / nrb, rblk = pidx % nrb;
  const int row0 = rblk * TK_RB;

  int mine = 0;
  if (tid < TK_RB) {
    const int row = row0 + tid;
    bool a = row < M;
    if (a && dom) a = (dom[row] != 0) == (which != 0);
    if (a && bad) a = bad[row] == 0;
    long t = -1;
    if (a && target) {
      t = target[row];
      if (t < 0) t += n;
      if (t < 0 || t >= n) t = -1;
    }
    act[tid] = a ? 1 : 0;
    tg[tid] = (int)t;
    cnt[tid] = 0;
    thr[tid] = -INFINITY;
    mine = a ? 1 : 0;
  }
  if (!__syncthreads_or(mine)) return;  // no row of this block passes the filter

  // stationary fragments: rows row0 + 32w + 16sb + l16 (clamped; rows past M are inactive)
  bf16x8 fh[2][KS], fl[2][KS];
#pragma unroll
  for (int sb = 0; sb < 2; ++sb) {
    const long sr = min(row0 + 32 * w + 16 * sb + l16, M - 1);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      fh[sb][ks] = *(const bf16x8*)(Qx + sr * D2 + ks * 32 + 8 * g);
      fl[sb][ks] = *(const bf16x8*)(Qx + sr * D2 + D + ks * 32 + 8 * g);
    }
  }
  bool arow[2];
#pragma unroll
  for (int sb = 0; sb < 2; ++sb) arow[sb] = act[32 * w + 16 * sb + l16] != 0;

  // tile loader: chunk c = p·256 + tid of the tile ↔ (row c / CPR, chunk c % CPR); LDS chunk ch of row r sits at
  // r·ROWB + 16·(ch ^ (r & 15)) (row fragments of 16 rows × one chunk column then cover all banks once)
  i32x4 stage[NLD];
  float bstage = 0.f;
  auto gload = [&](auto rowfn) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < NLD; ++p) {
      const int c = p * 256 + tid, r = c / CPR, ch = c % CPR;
      stage[p] = *(const i32x4*)((const char*)Wx + (long)rowfn(r) * ROWB + ch * 16);
    }
    if (tid < TK_T) bstage = bias[rowfn(tid)];
  };
  auto lstore = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < NLD; ++p) {
      const int c = p * 256 + tid, r = c / CPR, ch = c % CPR;
      *(i32x4*)(img[buf] + r * ROWB + 16 * (ch ^ (r & 15))) = stage[p];
    }
    if (tid < TK_T) bt[buf][tid] = bstage;
  };
  // S tile: acc[cb][sb][i] = swept row 16cb + 4g + i · stationary row 16sb + l16
  auto compute = [&](int buf, f32x4(&acc)[2][2]) __attribute__((always_inline)) {
    const char* base = img[buf];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int sb = 0; sb < 2; ++sb) acc[cb][sb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        const char* rp = base + (16 * cb + l16) * ROWB;
        const bf16x8 ah = *(const bf16x8*)(rp + 16 * ((4 * ks + g) ^ l16));
        const bf16x8 al = *(const bf16x8*)(rp + 16 * ((CPR / 2 + 4 * ks + g) ^ l16));
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) {
          acc[cb][sb] = TK_MF(ah, fh[sb][ks], acc[cb][sb]);
          acc[cb][sb] = TK_MF(al, fh[sb][ks], acc[cb][sb]);
          acc[cb][sb] = TK_MF(ah, fl[sb][ks], acc[cb][sb]);
        }
      }
    }
  };

  // ---- the targets' scores: gathered tile tt holds the target rows of block rows 32tt .. 32tt+31 (wave tt's
  // stationary rows); element (swept r, stationary r) is row r's target score
  float ts[2] = {INFINITY, INFINITY};
  if (target) {
    for (int tt = 0; tt < 4; ++tt) {
      gload([&](int r) { return max(tg[32 * tt + r], 0); });
      lstore(tt & 1);
      __syncthreads();
      if (tt == w) {
        f32x4 acc[2][2];
        compute(tt & 1, acc);
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) {
          const f32x4 a = acc[sb][sb];
          const int i = l16 & 3;
          const float d = i == 0 ? a[0] : i == 1 ? a[1] : i == 2 ? a[2] : a[3];
          const float v = d + bt[tt & 1][16 * sb + l16];
          ts[sb] = __shfl(v, (l16 >> 2) * 16 + l16, 64);
        }
      }
    }
    __syncthreads();
  }

  // ---- the sweep
  const int w_beg = (int)min((long)split * per_split, (long)n);
  const int w_end = (int)min((long)n, (long)w_beg + per_split);
  const int ntiles = (w_end - w_beg + TK_T - 1) / TK_T;
  u64* const L0 = lists + ((long)split * mpad + row0 + 32 * w) * cap;  // this wave's 32 lists
  int cgt[2] = {0, 0};
  if (ntiles > 0) {
    gload([&](int r) { return min(w_beg + r, n - 1); });
    lstore(0);
    __syncthreads();
  }
  for (int t = 0; t < ntiles; ++t) {
    const int buf = t & 1, j0 = w_beg + t * TK_T;
    if (t + 1 < ntiles) gload([&](int r) { return min(j0 + TK_T + r, n - 1); });
    f32x4 acc[2][2];
    compute(buf, acc);
    float th[2];
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) th[sb] = thr[32 * w + 16 * sb + l16];
    bool anyp = false;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      const f32x4 b4 = *(const f32x4*)&bt[buf][16 * cb + 4 * g];
#pragma unroll
      for (int sb = 0; sb < 2; ++sb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int j = j0 + 16 * cb + 4 * g + i;
          const float v = acc[cb][sb][i] + b4[i];
          const bool ok = j < w_end;
          cgt[sb] += ok && v > ts[sb] ? 1 : 0;
          if (ok && arow[sb] && v > th[sb]) {
            const int lr = 16 * sb + l16;  // row within the wave
            bool excl = false;
            if (exclude) {
              const int64_t* ex = exclude + (long)(row0 + 32 * w + lr) * E;
              for (int e = 0; e < E; ++e) excl = excl || ex[e] == (int64_t)j;
            }
            if (!excl) {
              const int pos = atomicAdd(&cnt[32 * w + lr], 1);
              if (pos < cap) L0[(long)lr * cap + pos] = tk_key(v, j);
              anyp = true;
            }
          }
        }
      }
    }
    if (__builtin_amdgcn_ballot_w64(anyp)) {
      // rows of this wave with fewer than one tile's worth of free slots: compact, raise the threshold
      wave_sync();
      const int c = lane < 32 ? cnt[32 * w + lane] : 0;
      u64 mask = __builtin_amdgcn_ballot_w64(c > cap - TK_T);
      while (mask) {
        const int r = __builtin_ctzll(mask);
        mask &= mask - 1;
        const int cr = min(__shfl(c, r, 64), cap);
        tk_compact(L0 + (long)r * cap, cr, k, scr[w], lane);
        if (lane == 0) {
          cnt[32 * w + r] = min(cr, k);
          if (cr >= k) thr[32 * w + r] = tk_score(scr[w][TK_CAPMAX]);
        }
        wave_sync();
      }
    }
    if (t + 1 < ntiles) lstore(buf ^ 1);
    __syncthreads();
  }

  // ---- this split's partial results: each row's list sorted down to its k best, the fill count, the rank count
  wave_sync();
  for (int r = 0; r < 32; ++r) {
    const int cr = min(cnt[32 * w + r], cap);
    if (cr > 0) tk_compact(L0 + (long)r * cap, cr, k, scr[w], lane);
    if (lane == 0) pcnt[(long)split * mpad + row0 + 32 * w + r] = min(cr, k);
  }
#pragma unroll
  for (int sb = 0; sb < 2; ++sb) {
    int x = cgt[sb];
    x += __shfl_xor(x, 16, 64);
    x += __shfl_xor(x, 32, 64);
    if (g == 0) rcnt[(long)split * mpad + row0 + 32 * w + 16 * sb + l16] = x;
  }
}

// One wave per row: the k best keys of the union of the splits' lists (split by split: the k best of (the k best so
// far ∪ the next list)), decoded; rank = 1 + Σ of the splits' counts.
__global__ __launch_bounds__(64) void topk_merge_kernel(const u64* __restrict__ lists, const int* __restrict__ pcnt,
                                                        const int* __restrict__ rcnt, int M, int n, int k, int cap,
                                                        int n_split, int mpad, const int64_t* __restrict__ target,
                                                        const int64_t* __restrict__ dom, int which,
                                                        const int* __restrict__ bad, int64_t* __restrict__ ids,
                                                        float* __restrict__ scores, int* __restrict__ rank) {
  __shared__ u64 A[TK_CAPMAX], Bk[TK_KMAX];
  const int row = blockIdx.x, lane = threadIdx.x;
  if (dom && ((dom[row] != 0) != (which != 0))) return;
  if (bad && bad[row] != 0) {
    for (int r = lane; r < k; r += 64) {
      ids[(long)row * k + r] = -1;
      scores[(long)row * k + r] = -INFINITY;
    }
    if (rank && lane == 0) rank[row] = -1;
    return;
  }
  int ncur = 0;
  for (int s = 0; s < n_split; ++s) {
    const long o = (long)s * mpad + row;
    const int c = min(max(pcnt[o], 0), k);
    if (c == 0) continue;
    for (int e = lane; e < ncur; e += 64) A[e] = Bk[e];
    for (int e = lane; e < c; e += 64) A[ncur + e] = lists[o * cap + e];
    const int tot = ncur + c;
    __syncthreads();
    for (int e = lane; e < tot; e += 64) {
      const u64 me = A[e];
      int r = 0;
      for (int f = 0; f < tot; ++f) r += A[f] > me ? 1 : 0;
      if (r < k) Bk[r] = me;
    }
    ncur = min(tot, k);
    __syncthreads();
  }
  for (int r = lane; r < k; r += 64) {
    const bool have = r < ncur;
    ids[(long)row * k + r] = have ? (int64_t)tk_id(Bk[r]) : (int64_t)-1;
    scores[(long)row * k + r] = have ? tk_score(Bk[r]) : -INFINITY;
  }
  if (rank && lane == 0) {
    long t = target ? target[row] : -1;
    if (target && t < 0) t += n;
    int rk = -1;
    if (target && t >= 0 && t < n) {
      rk = 1;
      for (int s = 0; s < n_split; ++s) rk += rcnt[(long)s * mpad + row];
    }
    rank[row] = rk;
  }
}

// out[r] = [RNE(x[r]) ‖ RNE(x[r] − RNE(x[r]))] with the d columns of x zero-padded to D; zero rows up to rows_out
__global__ void split_bf16_pad_kernel(const float* __restrict__ x, long rows, int d, int D, long rows_out,
                                      bf16* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows_out * D) return;
  const long r = i / D;
  const int c = (int)(i % D);
  const float v = r < rows && c < d ? x[r * d + c] : 0.f;
  const bf16 h = (bf16)v;
  out[r * 2 * D + c] = h;
  out[r * 2 * D + D + c] = (bf16)(v - (float)h);
}

// the head of eval_rank_kernel (eval.hip): q = h_share[i, L-1] + h_dom[i, idx_last_dom[i]], one wave per row
__global__ __launch_bounds__(64) void eval_query_kernel(const float* __restrict__ hs, const float* __restrict__ ha,
                                                        const float* __restrict__ hb, int L, int d,
                                                        const int64_t* __restrict__ il_a,
                                                        const int64_t* __restrict__ il_b,
                                                        const int64_t* __restrict__ xory,
                                                        const int64_t* __restrict__ seq_a,
                                                        const int64_t* __restrict__ seq_b, int64_t n_item_a,
                                                        float* __restrict__ q, int* __restrict__ bad,
                                                        int64_t* __restrict__ seen) {
  const int i = blockIdx.x, tid = threadIdx.x;
  const bool da = xory[i] == 0;
  int64_t il = da ? il_a[i] : il_b[i];
  if (il < 0) il += L;
  const bool isbad = il < 0 || il >= L;
  if (tid == 0) bad[i] = isbad ? 1 : 0;
  if (isbad) {
    for (int c = tid; c < d; c += 64) q[(long)i * d + c] = 0.f;
  } else {
    const float* hl = hs + ((long)i * L + (L - 1)) * d;
    const float* hd = (da ? ha : hb) + ((long)i * L + il) * d;
    for (int c = tid; c < d; c += 64) q[(long)i * d + c] = hl[c] + hd[c];
  }
  if (seen) {
    for (int l = tid; l < L; l += 64)
      seen[(long)i * L + l] = da ? seq_a[(long)i * L + l] : seq_b[(long)i * L + l] - n_item_a;
  }
}

int g_ncu_tk = 0;
int num_cus_tk() {
  if (!g_ncu_tk) {
    int dev = 0, v = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev);
    g_ncu_tk = v > 0 ? v : 256;
  }
  return g_ncu_tk;
}

bool tk_shape_ok(int M, int n, int k, int n_split) {
  return M >= 0 && n >= 1 && n <= 0x7fffff00 && k >= 1 && k <= TK_KMAX && k <= n && n_split >= 1 &&
         n_split <= 65535;
}

}  // namespace

C2_API int c2dsr_full_topk_supported(int d) { return d == 64 || d == 128 || d == 256; }

C2_API int c2dsr_full_topk_splits(int M, int n) {
  if (M <= 0 || n <= 0) return 1;
  const int nrb = c2::ceil_div(M, TK_RB), tiles = c2::ceil_div(n, TK_T);
  return max(1, min(c2::ceil_div(num_cus_tk(), nrb), tiles));
}

C2_API size_t c2dsr_full_topk_workspace(int M, int n, int k, int n_split) {
  if (!tk_shape_ok(M, n, k, n_split)) return 0;
  const size_t mpad = (size_t)c2::ceil_div(M, TK_RB) * TK_RB;
  return (size_t)n_split * mpad * ((size_t)tk_cap(k) * 8 + 8);
}

C2_API int c2dsr_f32_split_bf16_pad(const float* x, long rows, int d, int D, long rows_out, void* out, void* stream) {
  if (rows_out == 0) return 0;
  if (d < 1 || d > D || rows > rows_out || rows < 0) return (int)hipErrorInvalidValue;
  split_bf16_pad_kernel<<<c2::ceil_div(rows_out * D, 256), 256, 0, (hipStream_t)stream>>>(x, rows, d, D, rows_out,
                                                                                          (bf16*)out);
  C2_CHECK_LAUNCH();
  return 0;
}

C2_API int c2dsr_eval_query(const float* h_share, const float* h_a, const float* h_b, int B, int L, int d,
                            const int64_t* idx_last_a, const int64_t* idx_last_b, const int64_t* xory,
                            const int64_t* seq_a, const int64_t* seq_b, int64_t n_item_a, float* q, int* bad,
                            int64_t* seen, void* stream) {
  if (B < 0 || L <= 0 || d <= 0 || !q || !bad || (seen && (!seq_a || !seq_b))) return (int)hipErrorInvalidValue;
  if (B == 0) return 0;
  eval_query_kernel<<<B, 64, 0, (hipStream_t)stream>>>(h_share, h_a, h_b, L, d, idx_last_a, idx_last_b, xory, seq_a,
                                                       seq_b, n_item_a, q, bad, seen);
  C2_CHECK_LAUNCH();
  return 0;
}

C2_API int c2dsr_full_topk(const void* Qx, const void* Wx, const float* bias, int M, int n, int D, int k, int n_split,
                           const int64_t* target, const int64_t* exclude, int E, const int64_t* dom, int which,
                           const int* bad, int64_t* ids, float* scores, int* rank, void* ws, size_t ws_bytes,
                           void* stream) {
  if (!tk_shape_ok(M, n, k, n_split) || !c2dsr_full_topk_supported(D) || E < 0 || (exclude && E == 0) ||
      (which != 0 && which != 1) || (rank && !target))
    return (int)hipErrorInvalidValue;
  if (M == 0) return 0;
  const size_t need = c2dsr_full_topk_workspace(M, n, k, n_split);
  if (!Qx || !Wx || !bias || !ids || !scores || !ws || ws_bytes < need) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int nrb = c2::ceil_div(M, TK_RB), mpad = nrb * TK_RB, cap = tk_cap(k);
  const int per = c2::ceil_div(c2::ceil_div(n, TK_T), n_split) * TK_T;
  u64* lists = (u64*)ws;
  int* pcnt = (int*)(lists + (size_t)n_split * mpad * cap);
  int* rcnt = pcnt + (size_t)n_split * mpad;
  // (a block that the row filter skips leaves its counts unwritten; the merge reads none of its rows either)
  const dim3 grid(nrb * n_split);
#define TK_LAUNCH(DD)                                                                                              \
  topk_sweep_kernel<DD><<<grid, 256, 0, st>>>((const bf16*)Qx, (const bf16*)Wx, bias, M, n, k, cap, per, target,   \
                                              exclude, E, dom, which, bad, lists, pcnt, rcnt, mpad)
  if (D == 64)
    TK_LAUNCH(64);
  else if (D == 128)
    TK_LAUNCH(128);
  else
    TK_LAUNCH(256);
#undef TK_LAUNCH
  C2_CHECK_LAUNCH();
  topk_merge_kernel<<<M, 64, 0, st>>>(lists, pcnt, rcnt, M, n, k, cap, n_split, mpad, target, dom, which, bad, ids,
                                      scores, rank);
  C2_CHECK_LAUNCH();
  return 0;
}
