// Online evaluation of a segmentation validation step (gfx950): hard tp / fp / fn counts per class in one pass over the logits.
// Reference: nnunetv2/training/nnUNetTrainer/nnUNetTrainer.py:933-975 (validation_step: argmax + one-hot scatter, or sigmoid > 0.5, the
// ignore mask, get_tp_fp_fn_tn over axes [0, 2, 3, 4]) and nnunetv2/training/loss/dice.py:150-192 (get_tp_fp_fn_tn).
// Logits fp32 [B][K][N] (N = D H W, class-major: what am_seg_head writes); the target is read through element strides, as in loss_ops.hip.
// Every count is an integer from the first compare to the table: nothing passes through a float, so the result does not depend on the
// order of execution.  Nothing is ever indexed by a label or by the predicted class (both are only COMPARED with the class at hand).
//   seg_counts_tile   one workgroup per (sample, tile of 256 voxels): lane l owns the voxels 4l..4l+3 of the tile (one 16-byte load per
//                     class), wave w the classes w, w + 4, ...   softmax: one sweep keeps a running (max, argmax) per voxel with a strict >
//                     in ascending k (the first index of the maximum); the 4 waves' pairs meet in LDS, larger max wins, equal max goes to
//                     the smaller k.  Then per class three ballots per voxel slot over the wave's 256 voxels (predicted, labelled, both) and
//                     lane 0 writes one int32 x 4 partial {tp, fp, fn, 0} per (tile, class).  sigmoid: the prediction is x_k > 0 (sigmoid(x)
//                     > 0.5 without the exponential), one sweep, the same ballots.
//   seg_counts_fold   partial rows -> the int64 table [K][3]: a workgroup adds one chunk of rows for 16 classes in int64 and adds its
//                     three sums per class to the table with 64-bit integer atomics (exact in any order; at most 512 per address).
#include "common.h"
#include "../../include/anatomask_hip.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;
constexpr int CT = AM_SEG_COUNTS_TILE;                    // voxels per workgroup: 64 lanes x 4
static_assert(CT == 256, "one 16-byte load per lane of a wave");
constexpr int NO_CLASS = 0x7fffffff;                      // the argmax of a wave that has seen no class (K < 4) or no logit above -inf

struct CountArgs {
  const float* x; int B, K, D, H, W; long N;
  const void* tgt; long sb, sc, sd, sh, sw; int has_ignore, ignore_label;
  int vec;                                                // every class row is 16-byte aligned (N % 4 == 0 and the base pointer is)
  long rows;                                              // tiles per sample
  i32x4* partials;                                        // [B][rows][K]
  unsigned long long* table;                              // the tools-only atomic form (AM_ABLATE) adds here instead
  int dbg;
};

// the lane's 4 voxels v .. v + 3: how many of them exist, and their element offsets in the (strided) target
__device__ __forceinline__ void vox_setup(const CountArgs& a, long v, int& nv, long (&toff)[4]) {
  const long left = a.N - v;
  nv = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
  const long hw = (long)a.H * a.W;
  int d = (int)(v / hw);
  const long r = v - (long)d * hw;
  int h = (int)(r / a.W);
  int w = (int)(r - (long)h * a.W);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    toff[i] = d * a.sd + h * a.sh + w * a.sw;             // dereferenced only for i < nv
    if (++w == a.W) { w = 0; if (++h == a.H) { h = 0; ++d; } }
  }
}

__device__ __forceinline__ void ld4(const float* __restrict__ row, long v, int nv, bool vec, float (&x)[4]) {
  if (vec && nv == 4) {
    const f32x4 t = __builtin_nontemporal_load((const f32x4*)(row + v));      // read once: nothing to keep in the caches
    x[0] = t[0]; x[1] = t[1]; x[2] = t[2]; x[3] = t[3];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = i < nv ? row[v + i] : 0.f;
  }
}

__device__ __forceinline__ int wave_count(bool p) { return __popcll(__ballot(p)); }

// the three counts of class k over the wave's 256 voxels, from per-lane predicates (pred: predicted and counted, lab: labelled and counted)
__device__ __forceinline__ void emit(const CountArgs& a, i32x4* prow, int k, int lane, const bool (&pred)[4], const bool (&lab)[4]) {
  int np = 0, nl = 0, tp = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    np += wave_count(pred[i]);
    nl += wave_count(lab[i]);
    tp += wave_count(pred[i] && lab[i]);
  }
  if (lane == 0) {
    if (AM_DBG(a, 1)) {                                   // tools only: integer atomics straight on the table, no partials
      if (tp) atomicAdd(a.table + 3 * (long)k, (unsigned long long)tp);
      if (np - tp) atomicAdd(a.table + 3 * (long)k + 1, (unsigned long long)(np - tp));
      if (nl - tp) atomicAdd(a.table + 3 * (long)k + 2, (unsigned long long)(nl - tp));
    } else {
      i32x4 t; t[0] = tp; t[1] = np - tp; t[2] = nl - tp; t[3] = 0;
      prow[k] = t;
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void seg_counts_tile_kernel(CountArgs a) {
  __shared__ f32x4 s_m[4][64];
  __shared__ i32x4 s_a[4][64];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.y, K = a.K;
  const long tile = blockIdx.x, v = tile * CT + 4 * lane;
  const bool vec = a.vec != 0;
  int nv; long toff[4];
  vox_setup(a, v, nv, toff);
  const float* xb = a.x + (long)b * K * a.N;
  i32x4* prow = a.partials + ((long)b * a.rows + tile) * K;

  if (MODE == AM_SEG_SOFTMAX) {
    // counted[i]: the voxel exists and is not ignored; y: its class, -1 for a label outside [0, K) (no class: it can only add to fp)
    bool counted[4]; int y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      counted[i] = false; y[i] = -1;
      if (i >= nv) continue;
      const int lab = ((const int16_t*)a.tgt)[b * a.sb + toff[i]];
      if (a.has_ignore && lab == a.ignore_label) continue;
      counted[i] = true;
      y[i] = (lab >= 0 && lab < K) ? lab : -1;
    }
    float mx[4]; int am[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { mx[i] = -INFINITY; am[i] = NO_CLASS; }
#pragma unroll 4
    for (int k = wv; k < K; k += 4) {
      float x[4];
      ld4(xb + (long)k * a.N, v, nv, vec, x);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (x[i] > mx[i]) { mx[i] = x[i]; am[i] = k; }    // strict: the first of equal maxima stays; a NaN never wins
    }
    f32x4 tm; i32x4 ta;
#pragma unroll
    for (int i = 0; i < 4; ++i) { tm[i] = mx[i]; ta[i] = am[i]; }
    s_m[wv][lane] = tm; s_a[wv][lane] = ta;
    __syncthreads();
    int pred[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float M = s_m[0][lane][i]; int A = s_a[0][lane][i];
#pragma unroll
      for (int j = 1; j < 4; ++j) {
        const float mj = s_m[j][lane][i]; const int aj = s_a[j][lane][i];
        if (mj > M || (mj == M && aj < A)) { M = mj; A = aj; }
      }
      pred[i] = counted[i] ? (A == NO_CLASS ? 0 : A) : -2;    // no logit above -inf: class 0, as torch.argmax; not counted: matches no class
    }
    for (int k = wv; k < K; k += 4) {
      bool p[4], l[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { p[i] = pred[i] == k; l[i] = y[i] == k; }      // y is -1 wherever the voxel is not counted
      emit(a, prow, k, lane, p, l);
    }
  } else {
    bool counted[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      counted[i] = i < nv;
      if (counted[i] && a.has_ignore && ((const uint8_t*)a.tgt)[b * a.sb + (long)K * a.sc + toff[i]] != 0) counted[i] = false;
    }
#pragma unroll 2
    for (int k = wv; k < K; k += 4) {
      float x[4];
      ld4(xb + (long)k * a.N, v, nv, vec, x);
      bool p[4], l[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool on = i < nv && ((const uint8_t*)a.tgt)[b * a.sb + (long)k * a.sc + toff[i]] != 0;
        p[i] = counted[i] && x[i] > 0.f;
        l[i] = counted[i] && on;
      }
      emit(a, prow, k, lane, p, l);
    }
  }
}

// partial rows [R][K] int32 x 4 -> table int64 [K][3].  Thread (rl, kc): class blockIdx.x * 16 + kc, the rows r0 + rl, r0 + rl + 16, ...
// of the chunk blockIdx.y; the 16 chains meet in LDS and one thread per class adds the chunk's sums to the table.
__global__ __launch_bounds__(256) void seg_counts_fold_kernel(const i32x4* __restrict__ partials, long R, long per, int K,
                                                              unsigned long long* __restrict__ table) {
  __shared__ long long s_r[16][16][3];
  const int kc = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int k = blockIdx.x * 16 + kc;
  const long r0 = (long)blockIdx.y * per, r1 = r0 + per < R ? r0 + per : R;
  long long acc[3] = {0, 0, 0};
  if (k < K) {
#pragma unroll 4
    for (long r = r0 + rl; r < r1; r += 16) {
      const i32x4 t = partials[r * K + k];
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[j] += t[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) s_r[rl][kc][j] = acc[j];
  __syncthreads();
  if (rl == 0 && k < K) {
    for (int r = 1; r < 16; ++r)
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[j] += s_r[r][kc][j];
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (acc[j]) atomicAdd(table + 3 * (long)k + j, (unsigned long long)acc[j]);
  }
}

}  // namespace

extern "C" {

int am_seg_hard_counts(int mode, const float* logits, int B, int K, int D, int H, int W, const void* target, long tsb, long tsc, long tsd,
                       long tsh, long tsw, int has_ignore, int ignore_label, void* workspace, long workspace_bytes, long* counts,
                       int accumulate, void* stream) {
  if (!logits || !target || !workspace || !counts || B <= 0 || K < 1 || D <= 0 || H <= 0 || W <= 0) return -1;
  if (mode != AM_SEG_SOFTMAX && mode != AM_SEG_SIGMOID) return -1;
  if (B > 65535) return -1;
  CountArgs a{};
  a.x = logits; a.B = B; a.K = K; a.D = D; a.H = H; a.W = W; a.N = (long)D * H * W;
  a.tgt = target; a.sb = tsb; a.sc = tsc; a.sd = tsd; a.sh = tsh; a.sw = tsw; a.has_ignore = has_ignore != 0; a.ignore_label = ignore_label;
  a.rows = (a.N + CT - 1) / CT;
  if (a.rows > 0xffffffL) return -1;                      // rows * 256 threads stays below 2^32
  const long R = (long)B * a.rows;
  if (workspace_bytes < R * K * (long)sizeof(i32x4)) return -1;
  if (((uintptr_t)workspace & 15) || ((uintptr_t)counts & 7)) return -1;
  a.partials = (i32x4*)workspace; a.table = (unsigned long long*)counts;
  a.vec = a.N % 4 == 0 && ((uintptr_t)logits & 15) == 0;
#ifdef AM_ABLATE
  { const char* e = getenv("AM_SEG_COUNTS_DBG"); a.dbg = e ? atoi(e) : 0; }
#endif
  hipStream_t st = (hipStream_t)stream;
  if (!accumulate) AM_HIP(hipMemsetAsync(counts, 0, (size_t)K * 3 * sizeof(long), st));
  const dim3 grid((unsigned)a.rows, (unsigned)B);
  if (mode == AM_SEG_SOFTMAX) AM_LAUNCH(seg_counts_tile_kernel<AM_SEG_SOFTMAX>, grid, dim3(256), 0, st, a);
  else AM_LAUNCH(seg_counts_tile_kernel<AM_SEG_SIGMOID>, grid, dim3(256), 0, st, a);
  AM_CHECK_LAUNCH();
  if (AM_DBG(a, 1)) return 0;
  long chunks = (R + 63) / 64;                            // 64 rows (4 per thread) per workgroup, at most 512 chunks
  if (chunks > 512) chunks = 512;
  const long per = (R + chunks - 1) / chunks;
  AM_LAUNCH(seg_counts_fold_kernel, dim3((unsigned)((K + 15) / 16), (unsigned)chunks), dim3(256), 0, st, a.partials, R, per, K, a.table);
  AM_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
