// The training step's query path between the encoder and the scorer (gfx950), paragraph (11) of include/mgcn_hip.h:
//   (a) the backward of the two query-row gathers all_ent[src], all_rel[rel]: out[idx[b], :] += d[b, :] with the addends of a row
//       added one after another in ascending b, bit for bit the sequential f32 loop -- a one-workgroup plan launch sorts the unique
//       keys idx << 12 | b in LDS, a fill launch zeroes the window, a sum launch gives every run of equal rows to the workgroup
//       of its first position, which walks the run with threads over columns;
//   (b) the trunk's tail hidden_drop -> bn2 -> relu on [B, O] with batch statistics, forward and backward, one launch each: a
//       workgroup owns 16 columns over all rows, so nothing crosses workgroups.
// No float atomics, no spinning, no workgroup waits on another: every sum has a fixed order, so the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>

#include "mgcn_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int MAX_BATCH = MGCN_QUERY_MAX_BATCH;
constexpr int KEY_BITS = 12;                          // b < 4096 in the low bits of a sort key
constexpr uint64_t BAD_KEY = 1ull << 63;              // an index outside [0, num_rows): sorted behind every row, never followed
constexpr int64_t MAX_ROWS = int64_t(1) << 50;
constexpr int SORT_TPB = 1024;
constexpr int TPB = 256;
static_assert(MAX_BATCH == 1 << KEY_BITS, "b must fit the low bits of a key");

// ------------------------------------------------------------------------------------------------ (a) row gradients
// plan: row_sorted[pos], b_sorted[pos] of the keys idx[b] << 12 | b in ascending order (a bitonic network over `padded`, the
// next power of two, filled up with all-ones keys). The keys are unique, so the plan is a function of idx alone.
__global__ __launch_bounds__(SORT_TPB) void rows_plan_kernel(int batch, int padded, int64_t num_rows, const int64_t *__restrict__ idx,
                                                             int64_t *__restrict__ row_sorted, int32_t *__restrict__ b_sorted) {
  __shared__ uint64_t key[MAX_BATCH];
  const int tid = threadIdx.x;
  for (int i = tid; i < padded; i += SORT_TPB) {
    uint64_t k = ~0ull;
    if (i < batch) {
      const int64_t n = idx[i];
      k = (n >= 0 && n < num_rows) ? ((uint64_t(n) << KEY_BITS) | uint64_t(i)) : (BAD_KEY | uint64_t(i));
    }
    key[i] = k;
  }
  __syncthreads();
  for (int k = 2; k <= padded; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < padded; i += SORT_TPB) {
        const int l = i ^ j;
        if (l > i) {                                  // every pair belongs to one thread
          const uint64_t a = key[i], b = key[l];
          const bool up = (i & k) == 0;
          if ((a > b) == up) {
            key[i] = b;
            key[l] = a;
          }
        }
      }
      __syncthreads();
    }
  for (int i = tid; i < batch; i += SORT_TPB) {
    const uint64_t k = key[i];
    row_sorted[i] = (k & BAD_KEY) ? int64_t(-1) : int64_t(k >> KEY_BITS);
    b_sorted[i] = int32_t(k & uint64_t(MAX_BATCH - 1));
  }
}

// zero fill of a window whose rows are ldo > dim apart: one wave per row, lanes over columns; the guard columns are not touched
__global__ __launch_bounds__(TPB) void rows_fill_window_kernel(int64_t num_rows, int dim, float *__restrict__ out, int64_t ldo) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t r = int64_t(blockIdx.x) * (TPB / 64) + wave; r < num_rows; r += int64_t(gridDim.x) * (TPB / 64))
    for (int c = lane; c < dim; c += 64) out[r * ldo + c] = 0.f;
}

// zero fill of n contiguous floats: scalars up to the first 16-byte boundary and for the last n % 4, float4 stores between
__global__ __launch_bounds__(TPB) void rows_fill_flat_kernel(int64_t n, float *__restrict__ out) {
  const int64_t head0 = int64_t((16u - (reinterpret_cast<uintptr_t>(out) & 15u)) & 15u) >> 2;
  const int64_t head = head0 < n ? head0 : n;
  const int64_t nv = (n - head) >> 2;
  const int64_t t = int64_t(blockIdx.x) * TPB + threadIdx.x, step = int64_t(gridDim.x) * TPB;
  f32x4 *__restrict__ v = reinterpret_cast<f32x4 *>(out + head);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int64_t i = t; i < nv; i += step) v[i] = zero;
  if (t < head) out[t] = 0.f;
  const int64_t tail = head + (nv << 2) + t;
  if (tail < n) out[tail] = 0.f;
}

// sum: workgroup `pos` owns the run of equal rows that starts at sorted position pos (any other position exits); thread t adds
// d[b, c] for the run's b in ascending order, columns c = t, t + 256, ..., starting from 0 as the sequential loop does
__global__ __launch_bounds__(TPB) void rows_sum_kernel(int batch, int dim, const int64_t *__restrict__ row_sorted,
                                                       const int32_t *__restrict__ b_sorted, const float *__restrict__ d, int64_t ldd,
                                                       float *__restrict__ out, int64_t ldo) {
  const int pos = blockIdx.x;
  const int64_t row = row_sorted[pos];
  if (row < 0 || (pos > 0 && row_sorted[pos - 1] == row)) return;
  int end = pos + 1;
  while (end < batch && row_sorted[end] == row) ++end;
  for (int c = threadIdx.x; c < dim; c += TPB) {
    float acc = 0.f;
    for (int k = pos; k < end; ++k) acc += d[int64_t(b_sorted[k]) * ldd + c];
    out[row * ldo + c] = acc;
  }
}

inline size_t rows_workspace(int64_t batch) { return (size_t(batch) * (sizeof(int64_t) + sizeof(int32_t)) + 15u) & ~size_t(15); }

// ------------------------------------------------------------------------------------------------ (c) candidate lists
// The backward of the candidate-list loss, paragraph (14) of include/mgcn_hip.h. A list position (b, j) is live iff
// uint64(cand[b, j]) - uint64(row0) < n_local: one unsigned comparison before any address of ent / d_ent / d_bias is formed.
constexpr int CB_CHUNK = 64;                          // list positions of a chunk (the forward's unit)
constexpr int CB_UNR = 16;                            // row loads in flight per lane

__device__ __forceinline__ int64_t cand_live_row(int64_t id, int64_t row0, int64_t n_local) {
  const uint64_t d = uint64_t(id) - uint64_t(row0);
  return d < uint64_t(n_local) ? int64_t(d) : int64_t(-1);
}

// dx[b, c] = sum over chunks ch ascending of s_ch, s_ch = sum over the chunk's live positions j ascending of g[b, j] ent[o_j, c],
// every product and every sum rounded to f32. Workgroup = (query, 64 columns); wave w takes chunks w, w + 4, ... in rounds of four,
// a lane holds one position's (row, g) of the chunk and one column; wave 0 folds a round's four sums into dx in chunk order.
__global__ __launch_bounds__(TPB) void cand_bwd_x_kernel(int64_t n_cand, int64_t n_local, int64_t row0, int dim,
                                                         const float *__restrict__ g, int64_t ldg, const int64_t *__restrict__ cand,
                                                         int64_t ldc, const float *__restrict__ ent, int64_t lde,
                                                         float *__restrict__ dx, int64_t ldx) {
  __shared__ float part[TPB / 64][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = blockIdx.x;
  const int c = blockIdx.y * 64 + lane;
  const bool col = c < dim;
  const int64_t chunks = (n_cand + CB_CHUNK - 1) / CB_CHUNK;
  float acc = 0.f;
  for (int64_t r0 = 0; r0 < chunks; r0 += TPB / 64) {
    const int64_t ch = r0 + wave;
    float s = 0.f;
    if (ch < chunks) {                                // wave-uniform
      const int64_t j = ch * CB_CHUNK + lane;
      int64_t o_l = -1;
      float g_l = 0.f;
      if (j < n_cand) {
        o_l = cand_live_row(cand[b * ldc + j], row0, n_local);
        g_l = g[b * ldg + j];
      }
      const int64_t left = n_cand - ch * CB_CHUNK;
      const int n = int(left < CB_CHUNK ? left : CB_CHUNK);
      for (int i0 = 0; i0 < n; i0 += CB_UNR) {
        float e[CB_UNR], gv[CB_UNR];
        bool ok[CB_UNR];
#pragma unroll
        for (int i = 0; i < CB_UNR; ++i) {            // (positions past n hold row -1)
          const int64_t o = __shfl(o_l, (i0 + i) & 63);
          gv[i] = __shfl(g_l, (i0 + i) & 63);
          ok[i] = o >= 0;
          e[i] = (ok[i] && col) ? ent[o * lde + c] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < CB_UNR; ++i)
          if (ok[i]) s = __fadd_rn(s, __fmul_rn(gv[i], e[i]));
      }
    }
    part[wave][lane] = s;
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int w = 0; w < TPB / 64; ++w)
        if (r0 + w < chunks) acc = __fadd_rn(acc, part[w][lane]);
    }
    __syncthreads();
  }
  if (wave == 0 && col) dx[b * ldx + c] = acc;
}

// The row of plan entry i (its flat position pos = b K + j looked up in cand and tested), or -1: nothing is followed unchecked
__device__ __forceinline__ int64_t plan_row(const int64_t *__restrict__ perm, int64_t i, int64_t total, int64_t n_cand,
                                            const int64_t *__restrict__ cand, int64_t ldc, int64_t row0, int64_t n_local,
                                            int64_t &b, int64_t &j) {
  const int64_t pos = perm[i];
  if (pos < 0 || pos >= total) return -1;
  b = pos / n_cand;
  j = pos - b * n_cand;
  return cand_live_row(cand[b * ldc + j], row0, n_local);
}

// d_ent[o, :] = sum of g[pos] x[b(pos), :], d_bias[o] = sum of g[pos] over the run of plan entries with row o, in plan order, each
// the sequential f32 loop from 0. One WAVE per plan entry: the wave of a run's first entry walks the run, every other one exits;
// lanes over columns, four column slabs (256 columns) per walk.
__global__ __launch_bounds__(TPB) void cand_bwd_ent_kernel(int64_t total, int64_t n_cand, int64_t n_local, int64_t row0, int dim,
                                                           const float *__restrict__ g, int64_t ldg, const int64_t *__restrict__ cand,
                                                           int64_t ldc, const int64_t *__restrict__ perm, int64_t n_live,
                                                           const float *__restrict__ x, int64_t ldx, float *__restrict__ d_ent,
                                                           int64_t lde, float *__restrict__ d_bias) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t i = int64_t(blockIdx.x) * (TPB / 64) + wave; i < n_live; i += int64_t(gridDim.x) * (TPB / 64)) {
    int64_t b = 0, j = 0, pb = 0, pj = 0;
    const int64_t row = plan_row(perm, i, total, n_cand, cand, ldc, row0, n_local, b, j);
    if (row < 0) continue;                            // wave-uniform
    if (i > 0 && plan_row(perm, i - 1, total, n_cand, cand, ldc, row0, n_local, pb, pj) == row) continue;
    const int slabs = d_ent ? (dim + 255) / 256 : 1;
    for (int sl = 0; sl < slabs; ++sl) {
      const int c0 = sl * 256 + lane;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, sb = 0.f;
      int64_t kb = b, kj = j;
      for (int64_t k = i;;) {
        const float gv = g[kb * ldg + kj];
        if (d_ent) {
          const float *xr = x + kb * ldx;
          const float x0 = c0 < dim ? xr[c0] : 0.f, x1 = c0 + 64 < dim ? xr[c0 + 64] : 0.f;
          const float x2 = c0 + 128 < dim ? xr[c0 + 128] : 0.f, x3 = c0 + 192 < dim ? xr[c0 + 192] : 0.f;
          a0 = __fadd_rn(a0, __fmul_rn(gv, x0));
          a1 = __fadd_rn(a1, __fmul_rn(gv, x1));
          a2 = __fadd_rn(a2, __fmul_rn(gv, x2));
          a3 = __fadd_rn(a3, __fmul_rn(gv, x3));
        }
        sb = __fadd_rn(sb, gv);
        if (++k >= n_live || plan_row(perm, k, total, n_cand, cand, ldc, row0, n_local, kb, kj) != row) break;
      }
      if (d_ent) {
        float *dr = d_ent + row * lde;
        if (c0 < dim) dr[c0] = a0;
        if (c0 + 64 < dim) dr[c0 + 64] = a1;
        if (c0 + 128 < dim) dr[c0 + 128] = a2;
        if (c0 + 192 < dim) dr[c0 + 192] = a3;
      }
      if (sl == 0 && d_bias && lane == 0) d_bias[row] = sb;
    }
  }
}

// ------------------------------------------------------------------------------------------------ (d) split runs
// cand_bwd_ent_kernel's sums with a long run cut into pieces of S plan entries counted from the run's OWN first entry, paragraph
// (18) of include/mgcn_hip.h: a piece's partial is that kernel's loop over its entries, a row is the sequential fold from +0 of
// its pieces' partials in piece order. Three launches: heads (which entries begin a piece), pieces (one wave per head; a run
// of one piece is written straight to its row, with the bits of cand_bwd_ent_kernel), fold (one wave per run of several pieces).
// The sorted keys are only ever COMPARED, to find a run's first entry without a scan; every address is formed from cand through
// plan_row, so keys that do not belong to the plan can give wrong sums and nothing else.
constexpr int SPLIT_MIN = 16, SPLIT_MAX = 65536;
constexpr uint8_t HEAD_NONE = 0, HEAD_FIRST = 1, HEAD_NEXT = 2;
constexpr int SPLIT_UNR = 8;                          // entries whose x rows are in flight per lane (four columns each)
constexpr int FOLD_UNR = 4;                           // pieces whose slot loads are in flight per lane

// the workspace: piece slots of dim + 1 floats (the row's columns, then the bias term), two per window of S plan entries; per
// window the first entry of the run of several pieces that begins in it, or -1; per plan entry its head mark
struct SplitWs {
  float *slot;
  int64_t *first;
  uint8_t *mark;
};

inline size_t up16(size_t n) { return (n + 15u) & ~size_t(15); }
inline int64_t split_windows(int64_t total, int64_t S) { return (total + S - 1) / S; }
inline size_t split_workspace(int64_t total, int dim, int64_t S) {
  const size_t w = size_t(split_windows(total, S));
  return up16(2 * w * (size_t(dim) + 1) * sizeof(float)) + up16(w * sizeof(int64_t)) + up16(size_t(total));
}
inline SplitWs split_carve(void *ws, int64_t total, int dim, int64_t S) {
  const size_t w = size_t(split_windows(total, S));
  char *p = static_cast<char *>(ws);
  SplitWs out;
  out.slot = reinterpret_cast<float *>(p);
  p += up16(2 * w * (size_t(dim) + 1) * sizeof(float));
  out.first = reinterpret_cast<int64_t *>(p);
  p += up16(w * sizeof(int64_t));
  out.mark = reinterpret_cast<uint8_t *>(p);
  return out;
}

// (a) heads: one THREAD per plan entry i. The run of i's row begins at the lowest s in [0, i] with keys[s] >= row * total (the
// keys are row * total + position, ascending): galloped backwards from i, then bisected; every index read lies in [0, i]. Entry
// i begins a piece iff (i - s) % S == 0. The thread of a window's first entry i = (w + 1) S also writes first[w], the one
// store to it: a run of more than S entries that begins in window w holds entry (w + 1) S, so that thread sees it or there is
// none (two such runs cannot begin within S entries of each other).
__global__ __launch_bounds__(TPB) void cand_split_heads_kernel(int64_t total, int64_t n_cand, int64_t n_local, int64_t row0, int S,
                                                               const int64_t *__restrict__ cand, int64_t ldc,
                                                               const int64_t *__restrict__ perm, const int64_t *__restrict__ keys,
                                                               int64_t n_live, uint8_t *__restrict__ mark,
                                                               int64_t *__restrict__ first) {
  for (int64_t i = int64_t(blockIdx.x) * TPB + threadIdx.x; i < n_live; i += int64_t(gridDim.x) * TPB) {
    int64_t b = 0, j = 0;
    const int64_t row = plan_row(perm, i, total, n_cand, cand, ldc, row0, n_local, b, j);
    const bool window = i > 0 && i % S == 0;
    uint8_t m = HEAD_NONE;
    int64_t begins = -1;
    if (row >= 0) {
      const int64_t target = row * total;             // (fits: the entry point checks (n_local + 1) total)
      int64_t hi = i, lo = -1;
      for (int64_t step = 1;; step <<= 1) {
        const int64_t p = hi - step;
        if (p < 0) break;
        if (keys[p] < target) {
          lo = p;
          break;
        }
        hi = p;
      }
      while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < target)
          lo = mid;
        else
          hi = mid;
      }
      const int64_t d = i - hi;
      if (d % S == 0) m = d == 0 ? HEAD_FIRST : HEAD_NEXT;
      if (window && d > 0 && d <= S && hi + S < n_live &&
          plan_row(perm, hi + S, total, n_cand, cand, ldc, row0, n_local, b, j) == row)
        begins = hi;
    }
    mark[i] = m;
    if (window) first[i / S - 1] = begins;
  }
}

// (b) pieces: one WAVE per plan entry, a head walks at most S entries of its run, every other wave exits. The walk takes 64
// entries at a time, a lane looking up one entry's (row, query, g); the entries up to the first one of another row are then
// added in plan order, lanes over columns, four column slabs per walk as in cand_bwd_ent_kernel. A first head whose run ends
// within its piece writes the row; any other head writes slot 2 (i / S) + (first head ? 1 : 0).
__global__ __launch_bounds__(TPB) void cand_split_piece_kernel(int64_t total, int64_t n_cand, int64_t n_local, int64_t row0, int dim,
                                                               int S, const float *__restrict__ g, int64_t ldg,
                                                               const int64_t *__restrict__ cand, int64_t ldc,
                                                               const int64_t *__restrict__ perm, int64_t n_live,
                                                               const float *__restrict__ x, int64_t ldx,
                                                               const uint8_t *__restrict__ mark, float *__restrict__ slot,
                                                               float *__restrict__ d_ent, int64_t lde, float *__restrict__ d_bias) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t i = int64_t(blockIdx.x) * (TPB / 64) + wave; i < n_live; i += int64_t(gridDim.x) * (TPB / 64)) {
    const uint8_t m = mark[i];
    if (m == HEAD_NONE) continue;                     // wave-uniform
    int64_t b = 0, j = 0;
    const int64_t row = plan_row(perm, i, total, n_cand, cand, ldc, row0, n_local, b, j);
    if (row < 0) continue;
    const int64_t lim = i + S < n_live ? i + S : n_live;
    const int slabs = d_ent ? (dim + 255) / 256 : 1;
    for (int sl = 0; sl < slabs; ++sl) {
      const int c0 = sl * 256 + lane;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, sb = 0.f;
      int64_t walked = 0;
      for (int64_t k0 = i; k0 < lim; k0 += 64) {
        const int64_t k = k0 + lane;
        int64_t kb = 0, kj = 0;
        bool mine = false;
        if (k < lim) mine = plan_row(perm, k, total, n_cand, cand, ldc, row0, n_local, kb, kj) == row;
        const float g_l = mine ? g[kb * ldg + kj] : 0.f;
        const int b_l = int(kb);                      // (batch < 2^31)
        const unsigned long long others = ~__ballot(mine);
        const int n = others ? __builtin_ctzll(others) : 64;
        for (int q0 = 0; q0 < n; q0 += SPLIT_UNR) {
          float gv[SPLIT_UNR], x0[SPLIT_UNR], x1[SPLIT_UNR], x2[SPLIT_UNR], x3[SPLIT_UNR];
#pragma unroll
          for (int u = 0; u < SPLIT_UNR; ++u) {
            const int q = (q0 + u) & 63;
            gv[u] = __shfl(g_l, q);
            const float *xr = x + int64_t(__shfl(b_l, q)) * ldx;
            const bool on = d_ent && q0 + u < n;      // (an entry past n is another run's or none: its query is not looked at)
            x0[u] = on && c0 < dim ? xr[c0] : 0.f;
            x1[u] = on && c0 + 64 < dim ? xr[c0 + 64] : 0.f;
            x2[u] = on && c0 + 128 < dim ? xr[c0 + 128] : 0.f;
            x3[u] = on && c0 + 192 < dim ? xr[c0 + 192] : 0.f;
          }
#pragma unroll
          for (int u = 0; u < SPLIT_UNR; ++u)
            if (q0 + u < n) {
              if (d_ent) {
                a0 = __fadd_rn(a0, __fmul_rn(gv[u], x0[u]));
                a1 = __fadd_rn(a1, __fmul_rn(gv[u], x1[u]));
                a2 = __fadd_rn(a2, __fmul_rn(gv[u], x2[u]));
                a3 = __fadd_rn(a3, __fmul_rn(gv[u], x3[u]));
              }
              sb = __fadd_rn(sb, gv[u]);
            }
        }
        walked += n;
        if (n < 64) break;
      }
      const bool more = walked == S && i + S < n_live && plan_row(perm, i + S, total, n_cand, cand, ldc, row0, n_local, b, j) == row;
      if (m == HEAD_FIRST && !more) {                 // the whole run: cand_bwd_ent_kernel's stores
        if (d_ent) {
          float *dr = d_ent + row * lde;
          if (c0 < dim) dr[c0] = a0;
          if (c0 + 64 < dim) dr[c0 + 64] = a1;
          if (c0 + 128 < dim) dr[c0 + 128] = a2;
          if (c0 + 192 < dim) dr[c0 + 192] = a3;
        }
        if (sl == 0 && d_bias && lane == 0) d_bias[row] = sb;
      } else {
        float *sr = slot + (2 * (i / S) + (m == HEAD_FIRST ? 1 : 0)) * (int64_t(dim) + 1);
        if (d_ent) {
          if (c0 < dim) sr[c0] = a0;
          if (c0 + 64 < dim) sr[c0 + 64] = a1;
          if (c0 + 128 < dim) sr[c0 + 128] = a2;
          if (c0 + 192 < dim) sr[c0 + 192] = a3;
        }
        if (sl == 0 && lane == 0) sr[dim] = sb;
      }
    }
  }
}

// (c) fold: one WAVE per window w with (w + 1) S < n_live. s = first[w] is followed only if it lies in the window and entries s
// and s + S name one live row, each looked up through plan_row; the run's heads s, s + S, ... are then checked 64 at a time,
// a lane per head, and the slots of the ones before the first head of another row are added in piece order from +0.
__global__ __launch_bounds__(TPB) void cand_split_fold_kernel(int64_t total, int64_t n_cand, int64_t n_local, int64_t row0, int dim,
                                                              int S, const int64_t *__restrict__ cand, int64_t ldc,
                                                              const int64_t *__restrict__ perm, int64_t n_live, int64_t windows,
                                                              const int64_t *__restrict__ first, const float *__restrict__ slot,
                                                              float *__restrict__ d_ent, int64_t lde, float *__restrict__ d_bias) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t width = int64_t(dim) + 1;
  for (int64_t w = int64_t(blockIdx.x) * (TPB / 64) + wave; w < windows; w += int64_t(gridDim.x) * (TPB / 64)) {
    const int64_t s = first[w];
    if (s < w * S || s >= (w + 1) * S || s + S >= n_live) continue;      // wave-uniform
    int64_t b = 0, j = 0;
    const int64_t row = plan_row(perm, s, total, n_cand, cand, ldc, row0, n_local, b, j);
    if (row < 0 || plan_row(perm, s + S, total, n_cand, cand, ldc, row0, n_local, b, j) != row) continue;
    int64_t pieces = 0;
    for (int64_t p0 = 0;; p0 += 64) {
      const int64_t h = s + (p0 + lane) * S;
      const bool mine = h < n_live && plan_row(perm, h, total, n_cand, cand, ldc, row0, n_local, b, j) == row;
      const unsigned long long others = ~__ballot(mine);
      const int n = others ? __builtin_ctzll(others) : 64;
      pieces += n;
      if (n < 64) break;
    }
    // piece p's head is entry s + p S of window s / S + p: slot 2 (s / S + p) + (p == 0), below 2 ceil(total / S) as s + p S < n_live
    const float *base = slot + 2 * (s / S) * width;
    for (int64_t c0 = (d_ent ? 0 : dim) + lane; c0 < width; c0 += 256) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      for (int64_t p0 = 0; p0 < pieces; p0 += FOLD_UNR) {
        float v0[FOLD_UNR], v1[FOLD_UNR], v2[FOLD_UNR], v3[FOLD_UNR];
#pragma unroll
        for (int u = 0; u < FOLD_UNR; ++u) {
          const int64_t p = p0 + u;
          const float *sr = base + (2 * p + (p == 0 ? 1 : 0)) * width;
          const bool on = p < pieces;
          v0[u] = on ? sr[c0] : 0.f;
          v1[u] = on && c0 + 64 < width ? sr[c0 + 64] : 0.f;
          v2[u] = on && c0 + 128 < width ? sr[c0 + 128] : 0.f;
          v3[u] = on && c0 + 192 < width ? sr[c0 + 192] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < FOLD_UNR; ++u)
          if (p0 + u < pieces) {
            a0 = __fadd_rn(a0, v0[u]);
            a1 = __fadd_rn(a1, v1[u]);
            a2 = __fadd_rn(a2, v2[u]);
            a3 = __fadd_rn(a3, v3[u]);
          }
      }
      const float acc[4] = {a0, a1, a2, a3};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int64_t c = c0 + 64 * t;
        if (c < dim) {
          if (d_ent) d_ent[row * lde + c] = acc[t];
        } else if (c == dim && d_bias) {
          d_bias[row] = acc[t];
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ (b) trunk tail
constexpr int CW = 16;                               // columns of a workgroup
constexpr int RL = TPB / CW;                          // row lanes: thread (ty, tx) walks rows ty, ty + RL, ... of column tx

// u = z keep inv_keep in the order of model._drawn_dropout: (x * mask) * (1 / keep)
__device__ __forceinline__ float dropped(float z, const uint8_t *__restrict__ keep, int64_t at, float inv_keep) {
  return keep ? (z * (keep[at] ? 1.f : 0.f)) * inv_keep : z;
}

// the sum of the RL row lanes of every column: a halving tree of fixed shape, the result handed to all lanes of the column
__device__ __forceinline__ float column_sum(float v, float *red, int ty, int tx) {
  red[ty * CW + tx] = v;
  __syncthreads();
  for (int w = RL / 2; w > 0; w >>= 1) {
    if (ty < w) red[ty * CW + tx] += red[(ty + w) * CW + tx];
    __syncthreads();
  }
  const float s = red[tx];
  __syncthreads();
  return s;
}

struct TailArgs {
  int batch, dim;
  const float *z;
  int64_t ldz;
  const uint8_t *keep;
  int64_t ldk;
  float inv_keep;
};

// res = (sum_b (u - mean)) / B: what the f32 mean leaves of the centred column. Rows that nearly coincide (two-row batches
// above all) cancel in u - mean down to the mean's own rounding error, which rstd then multiplies; (u - mean) - res sums to
// zero to the accuracy of the differences themselves. Forward and backward centre with the same expression.
__device__ __forceinline__ float centring_residual(const TailArgs &a, float mean, bool live, int c, float *red, int ty, int tx) {
  float s = 0.f;
  if (live)
    for (int b = ty; b < a.batch; b += RL) s += dropped(a.z[b * a.ldz + c], a.keep, b * a.ldk + c, a.inv_keep) - mean;
  return column_sum(s, red, ty, tx) / float(a.batch);
}

__global__ __launch_bounds__(TPB) void tail_fwd_kernel(TailArgs a, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                       float *__restrict__ running_mean, float *__restrict__ running_var,
                                                       float momentum, float eps, float *__restrict__ x, int64_t ldx,
                                                       float *__restrict__ saved, int64_t ldsv) {
  __shared__ float red[TPB];
  const int tx = threadIdx.x % CW, ty = threadIdx.x / CW;
  const int c = blockIdx.x * CW + tx;
  const bool live = c < a.dim;
  const float count = float(a.batch);
  float s = 0.f;
  if (live)
    for (int b = ty; b < a.batch; b += RL) s += dropped(a.z[b * a.ldz + c], a.keep, b * a.ldk + c, a.inv_keep);
  const float mean = column_sum(s, red, ty, tx) / count;
  const float res = centring_residual(a, mean, live, c, red, ty, tx);
  float q = 0.f;
  if (live)
    for (int b = ty; b < a.batch; b += RL) {
      const float dl = (dropped(a.z[b * a.ldz + c], a.keep, b * a.ldk + c, a.inv_keep) - mean) - res;
      q += dl * dl;
    }
  const float sq = column_sum(q, red, ty, tx);
  if (!live) return;
  const float var = sq / count;
  const float rstd = 1.0f / sqrtf(var + eps);
  const float g = gamma[c], be = beta[c];
  for (int b = ty; b < a.batch; b += RL) {
    const float u = dropped(a.z[b * a.ldz + c], a.keep, b * a.ldk + c, a.inv_keep);
    const float v = (((u - mean) - res) * rstd) * g + be;
    x[b * ldx + c] = v <= 0.f ? 0.f : v;              // (a NaN stays a NaN)
  }
  if (ty == 0) {
    saved[c] = mean;
    saved[ldsv + c] = rstd;
    running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * mean;
    running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (sq / (count - 1.0f));
  }
}

__global__ __launch_bounds__(TPB) void tail_bwd_kernel(TailArgs a, const float *__restrict__ x, int64_t ldx,
                                                       const float *__restrict__ saved, int64_t ldsv, const float *__restrict__ gamma,
                                                       const float *__restrict__ gx, int64_t ldg, float *__restrict__ gz, int64_t ldgz,
                                                       float *__restrict__ d_gamma, float *__restrict__ d_beta) {
  __shared__ float red[TPB];
  const int tx = threadIdx.x % CW, ty = threadIdx.x / CW;
  const int c = blockIdx.x * CW + tx;
  const bool live = c < a.dim;
  const float mean = live ? saved[c] : 0.f, rstd = live ? saved[ldsv + c] : 0.f;
  const float res = centring_residual(a, mean, live, c, red, ty, tx);
  float sb = 0.f, sg = 0.f;
  if (live)
    for (int b = ty; b < a.batch; b += RL) {
      const float ga = x[b * ldx + c] > 0.f ? gx[b * ldg + c] : 0.f;      // the forward's relu mask, from its own output
      const float uh = ((dropped(a.z[b * a.ldz + c], a.keep, b * a.ldk + c, a.inv_keep) - mean) - res) * rstd;
      sb += ga;
      sg += ga * uh;
    }
  const float db = column_sum(sb, red, ty, tx);
  const float dg = column_sum(sg, red, ty, tx);
  if (!live) return;
  if (ty == 0) {
    if (d_beta) d_beta[c] = db;
    if (d_gamma) d_gamma[c] = dg;
  }
  if (!gz) return;
  const float count = float(a.batch);
  const float k = gamma[c] * rstd, mb = db / count, mg = dg / count;
  for (int b = ty; b < a.batch; b += RL) {
    const float ga = x[b * ldx + c] > 0.f ? gx[b * ldg + c] : 0.f;
    const float uh = ((dropped(a.z[b * a.ldz + c], a.keep, b * a.ldk + c, a.inv_keep) - mean) - res) * rstd;
    const float gu = k * ((ga - mb) - uh * mg);
    gz[b * ldgz + c] = a.keep ? (gu * (a.keep[b * a.ldk + c] ? 1.f : 0.f)) * a.inv_keep : gu;
  }
}

// what both tail entry points check of the arguments they share; MGCN_OK, or the code with the message set
int check_tail(const char *what, int32_t batch, int32_t dim, const float *z, int64_t ldz, const uint8_t *keep, int64_t ldk,
               float inv_keep) {
  MGCN_REQUIRE(batch >= 0 && dim >= 1, "%s: bad sizes (batch = %d, dim = %d)", what, batch, dim);
  MGCN_REQUIRE(z, "%s: null pointer (z)", what);
  MGCN_REQUIRE(ldz >= dim && (!keep || ldk >= dim), "%s: leading dimension smaller than dim = %d", what, dim);
  MGCN_REQUIRE(std::isfinite(inv_keep) && inv_keep >= 0.f, "%s: inv_keep must be a finite number >= 0", what);
  if (batch < 2 || batch > MAX_BATCH)
    return mgcn::fail(MGCN_EUNSUPPORTED, "%s: batch = %d outside [2, %d] (batch statistics need more than one value per channel)", what,
                      batch, MAX_BATCH);
  return MGCN_OK;
}

}  // namespace

extern "C" size_t mgcn_query_rows_bwd_workspace(int32_t batch) {
  return (batch >= 1 && batch <= MAX_BATCH) ? rows_workspace(batch) : 0;
}

extern "C" int mgcn_query_rows_bwd(int32_t batch, int64_t num_rows, int32_t dim, const int64_t *idx_dev, const float *d_dev, int64_t ldd,
                                   float *out_dev, int64_t ldo, void *workspace_dev, size_t workspace_bytes, void *stream) {
  MGCN_REQUIRE(batch >= 0 && num_rows >= 1 && dim >= 1, "mgcn_query_rows_bwd: bad sizes (batch = %d, num_rows = %lld, dim = %d)", batch,
               (long long)num_rows, dim);
  MGCN_REQUIRE(idx_dev && d_dev && out_dev, "mgcn_query_rows_bwd: null pointer");
  MGCN_REQUIRE(ldd >= dim && ldo >= dim, "mgcn_query_rows_bwd: leading dimension smaller than dim = %d", dim);
  if (batch < 1 || batch > MAX_BATCH)
    return mgcn::fail(MGCN_EUNSUPPORTED, "mgcn_query_rows_bwd: batch = %d outside [1, %d]", batch, MAX_BATCH);
  if (num_rows > MAX_ROWS) return mgcn::fail(MGCN_EUNSUPPORTED, "mgcn_query_rows_bwd: more than 2^50 rows");
  MGCN_REQUIRE(workspace_dev && mgcn::aligned16(workspace_dev), "mgcn_query_rows_bwd: null pointer or misaligned workspace");
  MGCN_REQUIRE(workspace_bytes >= rows_workspace(batch), "mgcn_query_rows_bwd: workspace too small (%zu < %zu bytes)", workspace_bytes,
               rows_workspace(batch));
  hipStream_t s = static_cast<hipStream_t>(stream);
  int64_t *row_sorted = static_cast<int64_t *>(workspace_dev);
  int32_t *b_sorted = reinterpret_cast<int32_t *>(row_sorted + batch);
  int padded = 2;
  while (padded < batch) padded <<= 1;
  rows_plan_kernel<<<dim3(1), dim3(SORT_TPB), 0, s>>>(batch, padded, num_rows, idx_dev, row_sorted, b_sorted);
  MGCN_CHECK_LAUNCH("mgcn_query_rows_bwd (plan)");
  if (ldo == dim) {
    const int64_t n = num_rows * dim, groups = (n / 4 + TPB - 1) / TPB + 1;
    rows_fill_flat_kernel<<<dim3(unsigned(groups < 8192 ? groups : 8192)), dim3(TPB), 0, s>>>(n, out_dev);
  } else {
    const int64_t groups = (num_rows + TPB / 64 - 1) / (TPB / 64);
    rows_fill_window_kernel<<<dim3(unsigned(groups < 16384 ? groups : 16384)), dim3(TPB), 0, s>>>(num_rows, dim, out_dev, ldo);
  }
  MGCN_CHECK_LAUNCH("mgcn_query_rows_bwd (fill)");
  rows_sum_kernel<<<dim3(batch), dim3(TPB), 0, s>>>(batch, dim, row_sorted, b_sorted, d_dev, ldd, out_dev, ldo);
  MGCN_CHECK_LAUNCH("mgcn_query_rows_bwd (sum)");
  return MGCN_OK;
}

extern "C" int mgcn_conve_tail_fwd(int32_t batch, int32_t dim, const float *z_dev, int64_t ldz, const uint8_t *keep_dev, int64_t ldk,
                                   float inv_keep, const float *gamma_dev, const float *beta_dev, float *running_mean_dev,
                                   float *running_var_dev, float momentum, float eps, float *x_dev, int64_t ldx, float *saved_dev,
                                   int64_t ldsv, void *stream) {
  if (int rc = check_tail("mgcn_conve_tail_fwd", batch, dim, z_dev, ldz, keep_dev, ldk, inv_keep)) return rc;
  MGCN_REQUIRE(gamma_dev && beta_dev && running_mean_dev && running_var_dev && x_dev && saved_dev, "mgcn_conve_tail_fwd: null pointer");
  MGCN_REQUIRE(ldx >= dim && ldsv >= dim, "mgcn_conve_tail_fwd: leading dimension smaller than dim = %d", dim);
  MGCN_REQUIRE(momentum >= 0.f && momentum <= 1.f && eps >= 0.f, "mgcn_conve_tail_fwd: momentum must lie in [0, 1] and eps be >= 0");
  const TailArgs a = {batch, dim, z_dev, ldz, keep_dev, ldk, inv_keep};
  tail_fwd_kernel<<<dim3((dim + CW - 1) / CW), dim3(TPB), 0, static_cast<hipStream_t>(stream)>>>(
      a, gamma_dev, beta_dev, running_mean_dev, running_var_dev, momentum, eps, x_dev, ldx, saved_dev, ldsv);
  MGCN_CHECK_LAUNCH("mgcn_conve_tail_fwd");
  return MGCN_OK;
}

extern "C" int mgcn_conve_tail_bwd(int32_t batch, int32_t dim, const float *z_dev, int64_t ldz, const uint8_t *keep_dev, int64_t ldk,
                                   float inv_keep, const float *x_dev, int64_t ldx, const float *saved_dev, int64_t ldsv,
                                   const float *gamma_dev, const float *gx_dev, int64_t ldg, float *gz_dev, int64_t ldgz,
                                   float *d_gamma_dev, float *d_beta_dev, void *stream) {
  if (int rc = check_tail("mgcn_conve_tail_bwd", batch, dim, z_dev, ldz, keep_dev, ldk, inv_keep)) return rc;
  MGCN_REQUIRE(x_dev && saved_dev && gamma_dev && gx_dev, "mgcn_conve_tail_bwd: null pointer");
  MGCN_REQUIRE(ldx >= dim && ldsv >= dim && ldg >= dim && (!gz_dev || ldgz >= dim),
               "mgcn_conve_tail_bwd: leading dimension smaller than dim = %d", dim);
  if (!gz_dev && !d_gamma_dev && !d_beta_dev) return MGCN_OK;
  const TailArgs a = {batch, dim, z_dev, ldz, keep_dev, ldk, inv_keep};
  tail_bwd_kernel<<<dim3((dim + CW - 1) / CW), dim3(TPB), 0, static_cast<hipStream_t>(stream)>>>(
      a, x_dev, ldx, saved_dev, ldsv, gamma_dev, gx_dev, ldg, gz_dev, ldgz, d_gamma_dev, d_beta_dev);
  MGCN_CHECK_LAUNCH("mgcn_conve_tail_bwd");
  return MGCN_OK;
}

namespace {
// what both candidate-list backward entry points check of the arguments they share
int check_cand_bwd(const char *what, int32_t batch, int64_t n_cand, int64_t n_local, int64_t ent_row0, int32_t dim, const float *g,
                   int64_t ldg, const int64_t *cand, int64_t ldc) {
  MGCN_REQUIRE(batch >= 0 && n_cand >= 0 && n_local >= 0 && ent_row0 >= 0 && dim >= 1, "%s: bad sizes", what);
  MGCN_REQUIRE(batch < (int64_t(1) << 31) - 64 && n_cand < (int64_t(1) << 31) - 64 && n_local < (int64_t(1) << 31) - 64,
               "%s: sizes exceed int32", what);
  MGCN_REQUIRE(g && cand, "%s: null pointer", what);
  MGCN_REQUIRE(ldg >= n_cand && ldc >= n_cand, "%s: leading dimension too small", what);
  return MGCN_OK;
}
}  // namespace

extern "C" int mgcn_cand_bce_bwd_x(int32_t batch, int64_t n_cand, int64_t n_local, int64_t ent_row0, int32_t dim, const float *g_dev,
                                   int64_t ldg, const int64_t *cand_dev, int64_t ldc, const float *ent_dev, int64_t lde,
                                   float *dx_dev, int64_t ldx, void *stream) {
  if (int rc = check_cand_bwd("cand_bce_bwd_x", batch, n_cand, n_local, ent_row0, dim, g_dev, ldg, cand_dev, ldc)) return rc;
  MGCN_REQUIRE(ent_dev && dx_dev, "cand_bce_bwd_x: null pointer");
  MGCN_REQUIRE(lde >= dim && ldx >= dim, "cand_bce_bwd_x: leading dimension too small");
  if (batch == 0 || n_cand == 0 || n_local == 0) return MGCN_OK;
  cand_bwd_x_kernel<<<dim3(unsigned(batch), unsigned((dim + 63) / 64)), dim3(TPB), 0, static_cast<hipStream_t>(stream)>>>(
      n_cand, n_local, ent_row0, dim, g_dev, ldg, cand_dev, ldc, ent_dev, lde, dx_dev, ldx);
  MGCN_CHECK_LAUNCH("cand_bwd_x_kernel");
  return MGCN_OK;
}

extern "C" int mgcn_cand_bce_bwd_ent(int32_t batch, int64_t n_cand, int64_t n_local, int64_t ent_row0, int32_t dim, const float *g_dev,
                                     int64_t ldg, const int64_t *cand_dev, int64_t ldc, const int64_t *perm_dev, int64_t n_live,
                                     const float *x_dev, int64_t ldx, float *d_ent_dev, int64_t lde, float *d_bias_dev, void *stream) {
  if (int rc = check_cand_bwd("cand_bce_bwd_ent", batch, n_cand, n_local, ent_row0, dim, g_dev, ldg, cand_dev, ldc)) return rc;
  MGCN_REQUIRE(perm_dev && (!d_ent_dev || x_dev), "cand_bce_bwd_ent: null pointer");   // (x is read for d_ent only)
  MGCN_REQUIRE(!d_ent_dev || (ldx >= dim && lde >= dim), "cand_bce_bwd_ent: leading dimension too small");
  const int64_t total = int64_t(batch) * n_cand;
  MGCN_REQUIRE(n_live >= 0 && n_live <= total, "cand_bce_bwd_ent: n_live outside [0, batch * n_cand]");
  if (batch == 0 || n_cand == 0 || n_local == 0 || n_live == 0 || (!d_ent_dev && !d_bias_dev)) return MGCN_OK;
  const int64_t groups = (n_live + TPB / 64 - 1) / (TPB / 64);
  cand_bwd_ent_kernel<<<dim3(unsigned(groups < (int64_t(1) << 22) ? groups : (int64_t(1) << 22))), dim3(TPB), 0,
                        static_cast<hipStream_t>(stream)>>>(total, n_cand, n_local, ent_row0, dim, g_dev, ldg, cand_dev, ldc, perm_dev,
                                                            n_live, x_dev, ldx, d_ent_dev, lde, d_bias_dev);
  MGCN_CHECK_LAUNCH("cand_bwd_ent_kernel");
  return MGCN_OK;
}

extern "C" size_t mgcn_cand_bwd_ent_split_workspace(int32_t batch, int64_t n_cand, int32_t dim, int32_t run_split) {
  const int64_t lim = (int64_t(1) << 31) - 64;
  if (batch < 0 || n_cand < 0 || batch >= lim || n_cand >= lim || dim < 1 || run_split < SPLIT_MIN || run_split > SPLIT_MAX) return 0;
  return split_workspace(int64_t(batch) * n_cand, dim, run_split) + 16;     // (never 0 for sizes it takes: 0 is the refusal)
}

extern "C" int mgcn_cand_bce_bwd_ent_split(int32_t batch, int64_t n_cand, int64_t n_local, int64_t ent_row0, int32_t dim,
                                           const float *g_dev, int64_t ldg, const int64_t *cand_dev, int64_t ldc,
                                           const int64_t *perm_dev, int64_t n_live, const float *x_dev, int64_t ldx, float *d_ent_dev,
                                           int64_t lde, float *d_bias_dev, const int64_t *keys_dev, int32_t run_split, void *ws_dev,
                                           size_t ws_bytes, void *stream) {
  const char *what = "cand_bce_bwd_ent_split";
  if (int rc = check_cand_bwd(what, batch, n_cand, n_local, ent_row0, dim, g_dev, ldg, cand_dev, ldc)) return rc;
  MGCN_REQUIRE(perm_dev && keys_dev && (!d_ent_dev || x_dev), "%s: null pointer", what);
  MGCN_REQUIRE(!d_ent_dev || (ldx >= dim && lde >= dim), "%s: leading dimension too small", what);
  const int64_t total = int64_t(batch) * n_cand;
  MGCN_REQUIRE(n_live >= 0 && n_live <= total, "%s: n_live outside [0, batch * n_cand]", what);
  MGCN_REQUIRE(run_split >= SPLIT_MIN && run_split <= SPLIT_MAX, "%s: run_split = %d outside [%d, %d]", what, run_split, SPLIT_MIN,
               SPLIT_MAX);
  MGCN_REQUIRE(total == 0 || n_local + 1 <= INT64_MAX / total, "%s: the keys row * (batch * n_cand) + position overflow int64", what);
  const size_t need = mgcn_cand_bwd_ent_split_workspace(batch, n_cand, dim, run_split);
  MGCN_REQUIRE(ws_dev && mgcn::aligned16(ws_dev), "%s: null pointer or misaligned workspace", what);
  MGCN_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu < %zu bytes)", what, ws_bytes, need);
  if (batch == 0 || n_cand == 0 || n_local == 0 || n_live == 0 || (!d_ent_dev && !d_bias_dev)) return MGCN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const SplitWs ws = split_carve(ws_dev, total, dim, run_split);
  const int64_t cap = int64_t(1) << 22;
  const int64_t tgroups = (n_live + TPB - 1) / TPB, wgroups = (n_live + TPB / 64 - 1) / (TPB / 64);
  cand_split_heads_kernel<<<dim3(unsigned(tgroups < cap ? tgroups : cap)), dim3(TPB), 0, s>>>(
      total, n_cand, n_local, ent_row0, run_split, cand_dev, ldc, perm_dev, keys_dev, n_live, ws.mark, ws.first);
  MGCN_CHECK_LAUNCH("cand_split_heads_kernel");
  cand_split_piece_kernel<<<dim3(unsigned(wgroups < cap ? wgroups : cap)), dim3(TPB), 0, s>>>(
      total, n_cand, n_local, ent_row0, dim, run_split, g_dev, ldg, cand_dev, ldc, perm_dev, n_live, x_dev, ldx, ws.mark, ws.slot,
      d_ent_dev, lde, d_bias_dev);
  MGCN_CHECK_LAUNCH("cand_split_piece_kernel");
  const int64_t windows = (n_live - 1) / run_split;   // the windows w whose successor's first entry (w + 1) S exists
  if (windows > 0) {
    const int64_t fgroups = (windows + TPB / 64 - 1) / (TPB / 64);
    cand_split_fold_kernel<<<dim3(unsigned(fgroups < cap ? fgroups : cap)), dim3(TPB), 0, s>>>(
        total, n_cand, n_local, ent_row0, dim, run_split, cand_dev, ldc, perm_dev, n_live, windows, ws.first, ws.slot, d_ent_dev, lde,
        d_bias_dev);
    MGCN_CHECK_LAUNCH("cand_split_fold_kernel");
  }
  return MGCN_OK;
}
