// Fused Dice + CE / BCE segmentation loss with its logit gradient (gfx950).
// Reference: nnunetv2/training/loss/compound_losses.py:8-100 (DC_and_CE_loss, DC_and_BCE_loss), dice.py:58-116
// (MemoryEfficientSoftDiceLoss), robust_ce_loss.py:6-16, deep_supervision.py:4-35, nnUNetTrainer.py:342-365 (_build_loss).
// Logits fp32 [B][K][N] (N = D H W, class-major: what am_seg_head writes); the target is read through element strides.  All kernels are
// streaming kernels bound by HBM traffic; nothing is ever indexed by a label (a label is only COMPARED with the class at hand), so a label
// outside [0, K) cannot reach LDS or global memory.
//   seg_loss_sums   one workgroup per (sample, tile of 256 voxels): lane l owns the voxels 4l..4l+3 of the tile (one 16-byte load per
//                   class), wave w the classes w, w + 4, ...   softmax: sweep 1 keeps a running (max, sum) per voxel, the 4 waves'
//                   pairs meet in LDS -> (max, log of the rescaled sum), stored (8 bytes per voxel) for the gradient pass; sweep 2 re-reads the tile
//                   (K KB per workgroup: served by the caches) and forms p = exp((x - max) - log sum) and the per-class sums.  sigmoid: one sweep.
//                   Each class is summed over the wave's 256 voxels (DPP rows, two cross-row steps) and lane 0 writes one partial
//                   {sum p y m, sum p m, sum y m, CE / BCE numerator}; entry K of a row is {unmasked voxels, sum of m lse over
//                   voxels of no class, 0, 0}.  No atomics.
//   seg_loss_fold   partial rows -> fp64 sums [B][K + 1][4], rows added in a fixed order (16 interleaved chains, then those in order).
//   seg_loss_coef   the sums -> the scalar loss (added, weighted, to the running total), a_c / b_c per (sample, class), the CE scale.
//   seg_loss_grad   the same tiling: softmax sweep 1 forms T = sum_j p_j (a_j y_j + b_j) per voxel (4 waves meet in LDS), sweep 2 writes
//                   dlogit_k = s m (p_k (a_k y_k + b_k - T) + c (p_k - y_k)); sigmoid writes s m (p_k (1 - p_k)(a_k y_k + b_k) + c (p_k - y_k))
//                   in one sweep.  s = *gscale * weight (the upstream gradient stays on the device), c = w_ce / n.
#include "common.h"
#include "../../include/anatomask_hip.h"

namespace {

typedef __attribute__((ext_vector_type(2))) float f32x2;
constexpr int LT = AM_SEG_LOSS_TILE;                      // voxels per workgroup: 64 lanes x 4
static_assert(LT == 256, "one 16-byte load per lane of a wave");

struct LossArgs {
  const float* x; int B, K, D, H, W; long N;
  const void* tgt; long sb, sc, sd, sh, sw; int has_ignore, ignore_label;
  int vec;                                                // every class row is 16-byte aligned (N % 4 == 0 and the base pointers are)
  long rows;                                              // tiles per sample
  float* partials; float* lse;                            // sums: out.  grad: lse in
  const float* coef; const float* gscale; float weight; float* dx;
};

// the lane's 4 voxels v .. v + 3: how many of them exist, and their element offsets in the (strided) target
__device__ __forceinline__ void vox_setup(const LossArgs& a, long v, int& nv, long (&toff)[4]) {
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
    const f32x4 t = *(const f32x4*)(row + v);
    x[0] = t[0]; x[1] = t[1]; x[2] = t[2]; x[3] = t[3];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = i < nv ? row[v + i] : 0.f;
  }
}

__device__ __forceinline__ void st4(float* __restrict__ row, long v, int nv, bool vec, const float (&o)[4]) {
  if (vec && nv == 4) {
    f32x4 t; t[0] = o[0]; t[1] = o[1]; t[2] = o[2]; t[3] = o[3];
    __builtin_nontemporal_store(t, (f32x4*)(row + v));
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) if (i < nv) row[v + i] = o[i];
  }
}

// sum over the 64 lanes, in every lane: 4 DPP adds inside the rows of 16, then the 4 rows
__device__ __forceinline__ float wave_sum64(float v) {
  v = row16_sum(v);
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// mask m (1 = the voxel counts) and class y (-1: none) of the lane's voxels
template <int MODE>
__device__ __forceinline__ void vox_target(const LossArgs& a, int b, int nv, const long (&toff)[4], float (&m)[4], int (&y)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    m[i] = 0.f; y[i] = -1;
    if (i >= nv) continue;
    if (MODE == AM_SEG_SOFTMAX) {
      const int lab = ((const int16_t*)a.tgt)[b * a.sb + toff[i]];
      if (a.has_ignore && lab == a.ignore_label) continue;
      m[i] = 1.f;
      y[i] = (lab >= 0 && lab < a.K) ? lab : -1;          // a label outside [0, K): no class (the reference's scatter_ errors there)
    } else {
      const bool ign = a.has_ignore && ((const uint8_t*)a.tgt)[b * a.sb + (long)a.K * a.sc + toff[i]] != 0;
      m[i] = ign ? 0.f : 1.f;
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void seg_loss_sums_kernel(LossArgs a) {
  __shared__ f32x4 s_m[4][64], s_s[4][64];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.y, K = a.K;
  const long tile = blockIdx.x, v = tile * LT + 4 * lane;
  const bool vec = a.vec != 0;
  int nv; long toff[4];
  vox_setup(a, v, nv, toff);
  float m[4]; int y[4];
  vox_target<MODE>(a, b, nv, toff, m, y);
  const float* xb = a.x + (long)b * K * a.N;
  f32x4* prow = (f32x4*)a.partials + ((long)b * a.rows + tile) * (K + 1);
  float vM[4] = {0.f, 0.f, 0.f, 0.f}, vL[4] = {0.f, 0.f, 0.f, 0.f};    // lse = vM + vL: the maximum and the log of the rescaled sum

  if (MODE == AM_SEG_SOFTMAX) {
    float mx[4], s[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { mx[i] = -INFINITY; s[i] = 0.f; }
#pragma unroll 2
    for (int k = wv; k < K; k += 4) {
      float x[4];
      ld4(xb + (long)k * a.N, v, nv, vec, x);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float d = x[i] - mx[i];
        const float e = expf(-fabsf(d));
        s[i] = d > 0.f ? fmaf(s[i], e, 1.f) : s[i] + e;   // one exponential per element: the sum is rescaled when the maximum grows
        mx[i] = fmaxf(mx[i], x[i]);
      }
    }
    f32x4 tm, ts;
#pragma unroll
    for (int i = 0; i < 4; ++i) { tm[i] = mx[i]; ts[i] = s[i]; }
    s_m[wv][lane] = tm; s_s[wv][lane] = ts;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float M = s_m[0][lane][i];
#pragma unroll
      for (int j = 1; j < 4; ++j) M = fmaxf(M, s_m[j][lane][i]);
      float S = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) S += s_s[j][lane][i] * expf(s_m[j][lane][i] - M);   // a wave without classes (K < 4): 0 * exp(-inf) = 0
      vM[i] = M; vL[i] = logf(S);
    }
    if (wv == 0 && a.lse) {
      f32x2* lp = (f32x2*)a.lse + (long)b * a.N;
#pragma unroll
      for (int i = 0; i < 4; ++i) if (i < nv) { f32x2 t; t[0] = vM[i]; t[1] = vL[i]; lp[v + i] = t; }
    }
  }

  for (int k = wv; k < K; k += 4) {
    float x[4];
    ld4(xb + (long)k * a.N, v, nv, vec, x);
    float I = 0.f, P = 0.f, G = 0.f, C = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (MODE == AM_SEG_SOFTMAX) {
        const float lp = (x[i] - vM[i]) - vL[i];           // log p_k
        const float p = expf(lp);
        const float yk = y[i] == k ? m[i] : 0.f;
        I = fmaf(p, yk, I);
        P = fmaf(p, m[i], P);
        G += yk;
        C = fmaf(yk, -lp, C);
      } else {
        const bool on = i < nv && ((const uint8_t*)a.tgt)[b * a.sb + (long)k * a.sc + toff[i]] != 0;
        const float yk = on ? m[i] : 0.f;
        const float p = 1.f / (1.f + expf(-x[i]));
        const float bce = fmaxf(x[i], 0.f) - (on ? x[i] : 0.f) + log1pf(expf(-fabsf(x[i])));
        I = fmaf(p, yk, I);
        P = fmaf(p, m[i], P);
        G += yk;
        C = fmaf(bce, m[i], C);
      }
    }
    I = wave_sum64(I); P = wave_sum64(P); G = wave_sum64(G); C = wave_sum64(C);
    if (lane == 0) { f32x4 t; t[0] = I; t[1] = P; t[2] = G; t[3] = C; prow[k] = t; }
  }
  if (wv == 0) {
    float cnt = 0.f, nc = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      cnt += m[i];
      if (MODE == AM_SEG_SOFTMAX && m[i] != 0.f && y[i] < 0) nc += vM[i] + vL[i];     // a voxel of no class: CE = lse (the gradient p_k / n)
    }
    cnt = wave_sum64(cnt); nc = wave_sum64(nc);
    if (lane == 0) { f32x4 t; t[0] = cnt; t[1] = nc; t[2] = 0.f; t[3] = 0.f; prow[K] = t; }
  }
}

// partial rows [B][rows][K1][4] fp32 -> sums [B][K1][4] fp64.  Thread (rl, kc): class blockIdx.x * 16 + kc, rows rl, rl + 16, ... in
// order; then the 16 chains in order.  Nothing depends on timing: the same input gives the same bits.
__global__ __launch_bounds__(256) void seg_loss_fold_kernel(const float* __restrict__ partials, long rows, int K1, double* __restrict__ sums) {
  __shared__ double s_r[16][16][4];
  const int kc = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int k = blockIdx.x * 16 + kc, b = blockIdx.y;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (k < K1) {
    const f32x4* p = (const f32x4*)partials + (long)b * rows * K1 + k;
#pragma unroll 4
    for (long r = rl; r < rows; r += 16) {
      const f32x4 t = p[r * K1];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += (double)t[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) s_r[rl][kc][j] = acc[j];
  __syncthreads();
  if (rl == 0 && k < K1) {
    for (int r = 1; r < 16; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += s_r[r][kc][j];
    double* o = sums + ((long)b * K1 + k) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = acc[j];
  }
}

struct CoefArgs {
  const double* sums; int B, K, mode, batch_dice, do_bg, has_ignore;
  double n_all, smooth, w_dice, w_ce; float level_weight;
  float* coef; float* loss_level; float* loss_total;
};

// One workgroup.  coef [B][K][2] = (w_dice a_c, w_dice b_c) (batch Dice: the same pair in every sample), coef[2 B K] = w_ce / n.
__global__ __launch_bounds__(256) void seg_loss_coef_kernel(CoefArgs a) {
  __shared__ double s_red[3][256];
  const int tid = threadIdx.x, B = a.B, K = a.K, K1 = K + 1, k0 = a.do_bg ? 0 : 1;
  const double Cp = (double)(K - k0) * (a.batch_dice ? 1 : B);
  double dsum = 0.0, csum = 0.0, nsum = 0.0;
  for (long t = tid; t < (long)B * K; t += 256) {
    const int b = (int)(t / K), k = (int)(t - (long)b * K);
    const double* sp = a.sums + ((long)b * K1 + k) * 4;
    csum += sp[3];
    double I = sp[0], P = sp[1], G = sp[2];
    if (a.batch_dice) {
      I = P = G = 0.0;
      for (int bb = 0; bb < B; ++bb) {
        const double* q = a.sums + ((long)bb * K1 + k) * 4;
        I += q[0]; P += q[1]; G += q[2];
      }
    }
    double ca = 0.0, cb = 0.0;
    if (k >= k0) {
      const double num = 2.0 * I + a.smooth, raw = G + P + a.smooth, den = raw > 1e-8 ? raw : 1e-8;
      if (!a.batch_dice || b == 0) dsum += num / den;
      ca = a.w_dice * (-2.0 / (Cp * den));
      cb = raw > 1e-8 ? a.w_dice * num / (Cp * den * den) : 0.0;      // the clip is active: the denominator is a constant
    }
    a.coef[2 * t] = (float)ca;
    a.coef[2 * t + 1] = (float)cb;
  }
  for (int b = tid; b < B; b += 256) {
    const double* q = a.sums + ((long)b * K1 + K) * 4;
    nsum += q[0];
    csum += q[1];
  }
  s_red[0][tid] = dsum; s_red[1][tid] = csum; s_red[2][tid] = nsum;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o)
      for (int j = 0; j < 3; ++j) s_red[j][tid] += s_red[j][tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    dsum = s_red[0][0]; csum = s_red[1][0]; nsum = s_red[2][0];
    const double dice = -dsum / Cp;
    double n;
    if (a.mode == AM_SEG_SOFTMAX) n = nsum;               // the mean over the unmasked voxels
    else n = a.has_ignore ? (nsum > 1e-8 ? nsum : 1e-8) : a.n_all;
    const bool empty = a.mode == AM_SEG_SOFTMAX && nsum == 0.0;      // every voxel ignored: the reference skips the CE term
    const double ce = empty ? 0.0 : csum / n;
    const double loss = a.w_ce * ce + a.w_dice * dice;
    a.coef[2 * (long)B * K] = empty ? 0.f : (float)(a.w_ce / n);
    a.loss_level[0] = (float)loss;
    if (a.loss_total) a.loss_total[0] += (float)((double)a.level_weight * loss);
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void seg_loss_grad_kernel(LossArgs a) {
  __shared__ f32x4 s_t[4][64];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.y, K = a.K;
  const long tile = blockIdx.x, v = tile * LT + 4 * lane;
  const bool vec = a.vec != 0;
  int nv; long toff[4];
  vox_setup(a, v, nv, toff);
  float m[4]; int y[4];
  vox_target<MODE>(a, b, nv, toff, m, y);
  const float* xb = a.x + (long)b * K * a.N;
  float* ob = a.dx + (long)b * K * a.N;
  const float* cf = a.coef + (long)b * K * 2;
  const float ces = a.coef[2 * (long)a.B * K];
  const float scale = a.gscale[0] * a.weight;
  float sm[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) sm[i] = scale * m[i];
  float vM[4] = {0.f, 0.f, 0.f, 0.f}, vL[4] = {0.f, 0.f, 0.f, 0.f}, T[4] = {0.f, 0.f, 0.f, 0.f};

  if (MODE == AM_SEG_SOFTMAX) {
    const f32x2* lp = (const f32x2*)a.lse + (long)b * a.N;
#pragma unroll
    for (int i = 0; i < 4; ++i) if (i < nv) { const f32x2 t = lp[v + i]; vM[i] = t[0]; vL[i] = t[1]; }
#pragma unroll 2
    for (int k = wv; k < K; k += 4) {
      float x[4];
      ld4(xb + (long)k * a.N, v, nv, vec, x);
      const float ak = cf[2 * k], bk = cf[2 * k + 1];
#pragma unroll
      for (int i = 0; i < 4; ++i) T[i] = fmaf(expf((x[i] - vM[i]) - vL[i]), y[i] == k ? ak + bk : bk, T[i]);
    }
    f32x4 t;
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = T[i];
    s_t[wv][lane] = t;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) T[i] = ((s_t[0][lane][i] + s_t[1][lane][i]) + s_t[2][lane][i]) + s_t[3][lane][i];
  }

#pragma unroll 2
  for (int k = wv; k < K; k += 4) {
    float x[4], o[4];
    ld4(xb + (long)k * a.N, v, nv, vec, x);
    const float ak = cf[2 * k], bk = cf[2 * k + 1];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (MODE == AM_SEG_SOFTMAX) {
        const float p = expf((x[i] - vM[i]) - vL[i]);
        const bool on = y[i] == k;
        o[i] = sm[i] * fmaf(p, (on ? ak + bk : bk) - T[i], ces * (p - (on ? 1.f : 0.f)));
      } else {
        const bool on = i < nv && ((const uint8_t*)a.tgt)[b * a.sb + (long)k * a.sc + toff[i]] != 0;
        const float p = 1.f / (1.f + expf(-x[i]));
        o[i] = sm[i] * fmaf(p * (1.f - p), on ? ak + bk : bk, ces * (p - (on ? 1.f : 0.f)));
      }
    }
    st4(ob + (long)k * a.N, v, nv, vec, o);
  }
}

// shared argument checks and geometry of the two big passes; 0 or -2
inline int loss_args(LossArgs& a, int mode, const float* logits, int B, int K, int D, int H, int W, const void* target, long tsb, long tsc,
                     long tsd, long tsh, long tsw, int has_ignore, int ignore_label) {
  if (!logits || !target || B <= 0 || K <= 0 || D <= 0 || H <= 0 || W <= 0) return -2;
  if (mode != AM_SEG_SOFTMAX && mode != AM_SEG_SIGMOID) return -2;
  if (mode == AM_SEG_SOFTMAX && K < 2) return -2;
  if (B > 65535) return -2;
  a.x = logits; a.B = B; a.K = K; a.D = D; a.H = H; a.W = W; a.N = (long)D * H * W;
  a.tgt = target; a.sb = tsb; a.sc = tsc; a.sd = tsd; a.sh = tsh; a.sw = tsw; a.has_ignore = has_ignore != 0; a.ignore_label = ignore_label;
  a.rows = (a.N + LT - 1) / LT;
  if (a.rows > 0xffffffL) return -2;                      // rows * 256 threads stays below 2^32
  return 0;
}

}  // namespace

extern "C" {

int am_seg_loss_sums(int mode, const float* logits, int B, int K, int D, int H, int W, const void* target, long tsb, long tsc, long tsd,
                     long tsh, long tsw, int has_ignore, int ignore_label, float* partials, double* sums, float* lse, void* stream) {
  LossArgs a{};
  if (int rc = loss_args(a, mode, logits, B, K, D, H, W, target, tsb, tsc, tsd, tsh, tsw, has_ignore, ignore_label)) return rc;
  if (!partials || !sums) return -2;
  if ((((uintptr_t)partials | (uintptr_t)sums) & 15) || ((uintptr_t)lse & 7)) return -3;
  a.partials = partials; a.lse = lse;
  a.vec = a.N % 4 == 0 && ((uintptr_t)logits & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)a.rows, (unsigned)B);
  if (mode == AM_SEG_SOFTMAX) AM_LAUNCH(seg_loss_sums_kernel<AM_SEG_SOFTMAX>, grid, dim3(256), 0, st, a);
  else AM_LAUNCH(seg_loss_sums_kernel<AM_SEG_SIGMOID>, grid, dim3(256), 0, st, a);
  AM_CHECK_LAUNCH();
  AM_LAUNCH(seg_loss_fold_kernel, dim3((unsigned)((K + 1 + 15) / 16), (unsigned)B), dim3(256), 0, st, partials, a.rows, K + 1, sums);
  AM_CHECK_LAUNCH();
  return 0;
}

int am_seg_loss_coeffs(int mode, const double* sums, int B, int K, long N, int batch_dice, int do_bg, int has_ignore, double smooth,
                       double w_dice, double w_ce, float level_weight, float* coef, float* loss_level, float* loss_total, void* stream) {
  if (!sums || !coef || !loss_level || B <= 0 || K <= 0 || N <= 0) return -2;
  if (mode != AM_SEG_SOFTMAX && mode != AM_SEG_SIGMOID) return -2;
  if (mode == AM_SEG_SOFTMAX && K < 2) return -2;
  if (!do_bg && K < 2) return -2;
  CoefArgs a{sums, B, K, mode, batch_dice != 0, do_bg != 0, has_ignore != 0, (double)B * K * (double)N, smooth, w_dice, w_ce, level_weight,
             coef, loss_level, loss_total};
  AM_LAUNCH(seg_loss_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
  AM_CHECK_LAUNCH();
  return 0;
}

int am_seg_loss_grad(int mode, const float* logits, int B, int K, int D, int H, int W, const void* target, long tsb, long tsc, long tsd,
                     long tsh, long tsw, int has_ignore, int ignore_label, const float* lse, const float* coef, const float* gscale,
                     float weight, float* dlogits, void* stream) {
  LossArgs a{};
  if (int rc = loss_args(a, mode, logits, B, K, D, H, W, target, tsb, tsc, tsd, tsh, tsw, has_ignore, ignore_label)) return rc;
  if (!coef || !gscale || !dlogits || (mode == AM_SEG_SOFTMAX && !lse)) return -2;
  if ((uintptr_t)lse & 7) return -3;
  a.lse = const_cast<float*>(lse); a.coef = coef; a.gscale = gscale; a.weight = weight; a.dx = dlogits;
  a.vec = a.N % 4 == 0 && (((uintptr_t)logits | (uintptr_t)dlogits) & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)a.rows, (unsigned)B);
  if (mode == AM_SEG_SOFTMAX) AM_LAUNCH(seg_loss_grad_kernel<AM_SEG_SOFTMAX>, grid, dim3(256), 0, st, a);
  else AM_LAUNCH(seg_loss_grad_kernel<AM_SEG_SIGMOID>, grid, dim3(256), 0, st, a);
  AM_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
