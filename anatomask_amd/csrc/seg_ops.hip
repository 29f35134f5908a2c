// STUNet segmentation inference (gfx950): the four kernels of the sliding-window predictor that are not convolutions / norms.
// Reference: nnunetv2/inference/predict_from_raw_data.py:622-754 (predict_sliding_window_return_logits, _internal_maybe_mirror_and_predict)
// and P/STUNet.py:10-129 (the network).  All of them are streaming kernels bound by HBM traffic:
//   seg_gather   tile of the (implicitly zero-padded) volume -> [M][T0][T1][T2] fp32, one slice per mirror combination
//   seg_upcat    cat(nearest_up(u), skip) channels-last, 16-byte chunks
//   seg_head     1x1 conv C -> K: plain (class-major logits) or accumulate (sum of the un-flipped mirrors, Gaussian-weighted, into the
//                whole-volume accumulator; tiles run in order on one stream, no atomics: bitwise reproducible)
//   seg_finalize acc / wsum over the un-padded crop (+ argmax labels)
//   seg_export   the same crop and division, then softmax / sigmoid probabilities and argmax / region labels in one pass
//                (LabelManager.apply_inference_nonlin + convert_probabilities_to_segmentation, label_handling.py:128-175)
// Mirror m of a set of allowed axes (bit a of `axes` = spatial axis a): bit j of m flips the j-th allowed axis (ascending).  M = 2^popcount.
#include "common.h"
#include "../../include/anatomask_hip.h"

namespace {

// flip flags (bit a = axis a flipped) of mirror m
__device__ __forceinline__ int mirror_flips(int axes, int m) {
  int f = 0, j = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a)
    if (axes & (1 << a)) { if (m & (1 << j)) f |= 1 << a; ++j; }
  return f;
}

__global__ __launch_bounds__(256) void seg_gather_kernel(const float* __restrict__ vol, int X, int Y, int Z, int o0, int o1, int o2,
                                                         int T0, int T1, int T2, int axes, int M, float* __restrict__ out) {
  const long nt = (long)T0 * T1 * T2;
  const long n = nt * M;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int m = (int)(i / nt);
    long r = i - (long)m * nt;
    const int t2 = (int)(r % T2); r /= T2;
    const int t1 = (int)(r % T1);
    const int t0 = (int)(r / T1);
    const int f = mirror_flips(axes, m);
    const int x = o0 + ((f & 1) ? T0 - 1 - t0 : t0);
    const int y = o1 + ((f & 2) ? T1 - 1 - t1 : t1);
    const int z = o2 + ((f & 4) ? T2 - 1 - t2 : t2);
    float v = 0.f;
    if (x >= 0 && x < X && y >= 0 && y < Y && z >= 0 && z < Z) v = vol[((long)x * Y + y) * Z + z];
    out[i] = v;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void seg_upcat_kernel(const T* __restrict__ u, const T* __restrict__ skip, T* __restrict__ y, int B, int D,
                                                        int H, int W, int C, int factor) {
  constexpr int EPC = 16 / sizeof(T);
  const int cc = C / EPC;                                 // chunks per voxel of u / skip
  const int d = D / factor, h = H / factor, w = W / factor;
  const long nvox = (long)B * D * H * W;
  const long n = nvox * 2 * cc;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long v = i / (2 * cc);
    const int c = (int)(i - v * 2 * cc);
    u32x4 val;
    if (c < cc) {
      long r = v;
      const int iw = (int)(r % W); r /= W;
      const int ih = (int)(r % H); r /= H;
      const int id = (int)(r % D);
      const int b = (int)(r / D);
      const long src = (((long)b * d + id / factor) * h + ih / factor) * w + iw / factor;
      val = *(const u32x4*)(u + src * C + (long)c * EPC);
    } else {
      val = *(const u32x4*)(skip + v * C + (long)(c - cc) * EPC);
    }
    *(u32x4*)(y + i * EPC) = val;
  }
}

constexpr int HV = 64;                                    // voxels per workgroup of the head (one per lane, 4 waves split the classes)

struct HeadArgs {
  const void* f; int B, T0, T1, T2, C;                    // features [B][T0][T1][T2][C]; accumulate mode: B = M mirrors of one tile
  const float* w; const float* bias; int K;               // [K][C], [K]
  float* logits;                                          // plain: [B][K][T0][T1][T2]
  int axes; const float* gauss; float* acc; float* wsum; int X, Y, Z, s0, s1, s2;   // accumulate
};

// plain (acc == NULL): logits[b][k][v] = w_k . f[b][v] + b_k.
// accumulate: s[v] = sum_m f_m[unflip_m(v)] (fp32), val_k = (w_k . s + M b_k) / M, acc[k][tile origin + v] += val_k g[v], wsum += g[v].
// C <= AM_SEG_LDS_C: the voxels' (summed) features are staged in LDS as fp32 rows; wider plain heads (the coarse deep-supervision
// levels, at most a few thousand voxels) read their features straight from global memory.
template <typename T>
__global__ __launch_bounds__(256) void seg_head_kernel(HeadArgs a) {
  extern __shared__ float s_lds[];                        // [HV][C + 1]: padded rows, conflict-free dots
  const int C = a.C, CP = C + 1;
  const long nt = (long)a.T0 * a.T1 * a.T2;
  const bool accum = a.acc != nullptr, staged = C <= AM_SEG_LDS_C;
  const int M = accum ? a.B : 1;
  const long tiles_per_b = (nt + HV - 1) / HV;
  const int b = accum ? 0 : (int)(blockIdx.x / tiles_per_b);
  const long v0 = (long)(blockIdx.x - (long)b * tiles_per_b) * HV;
  const int tid = threadIdx.x;
  const T* f = (const T*)a.f;

  if (staged) {
    for (int e = tid; e < HV * C; e += 256) {
      const int vl = e / C, c = e - vl * C;
      const long v = v0 + vl;
      float s = 0.f;
      if (v < nt) {
        long r = v;
        const int t2 = (int)(r % a.T2); r /= a.T2;
        const int t1 = (int)(r % a.T1);
        const int t0 = (int)(r / a.T1);
        for (int m = 0; m < M; ++m) {
          const int fl = accum ? mirror_flips(a.axes, m) : 0;
          const int x = (fl & 1) ? a.T0 - 1 - t0 : t0, y = (fl & 2) ? a.T1 - 1 - t1 : t1, z = (fl & 4) ? a.T2 - 1 - t2 : t2;
          const long src = (long)(accum ? m : b) * nt + ((long)x * a.T1 + y) * a.T2 + z;
          s += TT<T>::ld(f + src * C + c);
        }
      }
      s_lds[vl * CP + c] = s;
    }
    __syncthreads();
  }

  const int vl = tid & (HV - 1), kg = tid >> 6;
  const long v = v0 + vl;
  if (v >= nt) return;
  const float* sv = s_lds + vl * CP;
  const T* fv = f + ((long)b * nt + v) * C;
  auto dot = [&](int k) {
    const float* wk = a.w + (long)k * C;
    float d = 0.f;
    if (staged) {
      for (int c = 0; c < C; ++c) d = fmaf(wk[c], sv[c], d);
    } else {
      for (int c = 0; c < C; ++c) d = fmaf(wk[c], TT<T>::ld(fv + c), d);
    }
    return d;
  };
  if (!accum) {
    float* out = a.logits + (long)b * a.K * nt + v;
    for (int k = kg; k < a.K; k += 4) out[(long)k * nt] = dot(k) + a.bias[k];
    return;
  }
  long r = v;
  const int t2 = (int)(r % a.T2); r /= a.T2;
  const int t1 = (int)(r % a.T1);
  const int t0 = (int)(r / a.T1);
  const long plane = (long)a.X * a.Y * a.Z;
  const long q = ((long)(a.s0 + t0) * a.Y + (a.s1 + t1)) * a.Z + (a.s2 + t2);
  const float g = a.gauss ? a.gauss[v] : 1.f;
  const float mf = (float)M, inv = 1.f / mf;              // M is a power of two: the division is exact
  for (int k = kg; k < a.K; k += 4) {
    float* p = a.acc + (long)k * plane + q;
    *p += fmaf(mf, a.bias[k], dot(k)) * inv * g;          // M == 1: (w_k . f + b_k) g exactly
  }
  if (kg == 0) a.wsum[q] += g;
}

template <typename L>
__global__ __launch_bounds__(256) void seg_finalize_kernel(const float* __restrict__ acc, const float* __restrict__ wsum, int K, int Xp, int Yp,
                                                           int Zp, int c0, int c1, int c2, int X, int Y, int Z, float* __restrict__ logits,
                                                           L* __restrict__ labels) {
  const long n = (long)X * Y * Z;
  const long plane = (long)Xp * Yp * Zp;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    long r = i;
    const int z = (int)(r % Z); r /= Z;
    const int y = (int)(r % Y);
    const int x = (int)(r / Y);
    const long q = ((long)(x + c0) * Yp + (y + c1)) * Zp + (z + c2);
    const float w = wsum[q];
    float best = 0.f; int arg = 0;
    for (int k = 0; k < K; ++k) {
      const float val = acc[(long)k * plane + q] / w;
      if (logits) logits[(long)k * n + i] = val;
      if (k == 0 || val > best) { best = val; arg = k; }       // strict >: the lowest index wins a tie (torch.argmax)
    }
    if (labels) labels[i] = (L)arg;
  }
}

constexpr int EV = 64;                                    // voxels per workgroup of the export (one per lane, 4 waves split the classes)
constexpr int EXPORT_LDS_K = 600;                         // softmax probabilities: the workgroup's K x EV logits stay in LDS up to this K

struct ExportArgs {
  const float* acc; const float* wsum; int K, Xp, Yp, Zp, c0, c1, c2, X, Y, Z;
  int nonlin; const int32_t* order; float* probs; void* labels; int staged;
};

// One workgroup owns EV consecutive voxels of the crop (grid-stride over such slabs); wave kg owns the classes kg, kg + 4, ...; lane v the
// voxel.  l_k = acc[k][q] / wsum[q] exactly as seg_finalize.
//   softmax: per-thread (max, argmax) -> 4-way combine through LDS (the lowest index wins a tie) -> labels; probabilities:
//     staged (K <= EXPORT_LDS_K): l_k were kept in LDS, e_k = expf(l_k - max) replaces them, S = sum of the 4 partial sums, p_k = e_k / S:
//       every accumulator element is read once;
//     otherwise the first pass keeps a running (max, sum) per thread (rescaled when the max grows), the partials are rescaled to the common
//       max, and a second read of the accumulator writes expf(l_k - max) / S;
//   sigmoid: p_k = 1 / (1 + expf(-l_k)); label = order[highest k with p_k > 0.5], 0 when there is none (the reference's in-order overwrite).
template <typename L>
__global__ __launch_bounds__(256) void seg_export_kernel(ExportArgs a) {
  extern __shared__ float s_lds[];
  float* red_f = s_lds;                                   // [4][EV]
  int* red_i = (int*)(s_lds + 4 * EV);                    // [4][EV]
  float* sl = s_lds + 8 * EV;                             // [K][EV], staged only
  const int K = a.K;
  const long n = (long)a.X * a.Y * a.Z;
  const long plane = (long)a.Xp * a.Yp * a.Zp;
  const long slabs = (n + EV - 1) / EV;
  const int lane = threadIdx.x & (EV - 1), kg = threadIdx.x >> 6;
  const bool staged = a.staged != 0;
  L* labels = (L*)a.labels;
  for (long t = blockIdx.x; t < slabs; t += gridDim.x) {
    const long i = t * EV + lane;
    const bool valid = i < n;
    long q = 0;
    float w = 1.f;
    if (valid) {
      long r = i;
      const int z = (int)(r % a.Z); r /= a.Z;
      const int y = (int)(r % a.Y);
      const int x = (int)(r / a.Y);
      q = ((long)(x + a.c0) * a.Yp + (y + a.c1)) * a.Zp + (z + a.c2);
      w = a.wsum[q];
    }
    const float* ap = a.acc + q;
    float* pp = a.probs + i;                              // (dereferenced only when a.probs and valid)
    if (a.nonlin == AM_SEG_SIGMOID) {
      int last = -1;
      if (valid)
        for (int k = kg; k < K; k += 4) {
          const float p = 1.f / (1.f + expf(-(ap[(long)k * plane] / w)));
          if (a.probs) pp[(long)k * n] = p;
          if (p > 0.5f) last = k;
        }
      if (labels) {
        red_i[kg * EV + lane] = last;
        __syncthreads();
        if (kg == 0 && valid) {
          for (int j = 1; j < 4; ++j) last = max(last, red_i[j * EV + lane]);
          labels[i] = last < 0 ? (L)0 : (L)a.order[last];
        }
        __syncthreads();
      }
      continue;
    }
    float m = -INFINITY, s = 0.f;
    int arg = 0x7fffffff;
    if (valid)
      for (int k = kg; k < K; k += 4) {
        const float l = ap[(long)k * plane] / w;
        if (staged) sl[k * EV + lane] = l;
        const bool up = k == kg || l > m;                 // strict >: the lowest index wins a tie (torch.argmax)
        if (a.probs && !staged) s = up ? s * expf(m - l) + 1.f : s + expf(l - m);
        if (up) { m = l; arg = k; }
      }
    red_f[kg * EV + lane] = m;
    red_i[kg * EV + lane] = arg;
    __syncthreads();
    float mx = red_f[lane];
    int am = red_i[lane];
    for (int j = 1; j < 4; ++j) {
      const float mj = red_f[j * EV + lane];
      const int aj = red_i[j * EV + lane];
      if (mj > mx || (mj == mx && aj < am)) { mx = mj; am = aj; }
    }
    if (labels && kg == 0 && valid) labels[i] = (L)am;
    if (a.probs) {
      float ps = 0.f;
      if (staged) {
        if (valid)
          for (int k = kg; k < K; k += 4) {
            const float e = expf(sl[k * EV + lane] - mx);
            sl[k * EV + lane] = e;
            ps += e;
          }
      } else if (s != 0.f) {
        ps = s * expf(m - mx);
      }
      __syncthreads();                                    // every thread has read the (max, argmax) partials
      red_f[kg * EV + lane] = ps;
      __syncthreads();
      const float S = ((red_f[lane] + red_f[EV + lane]) + red_f[2 * EV + lane]) + red_f[3 * EV + lane];
      if (valid)
        for (int k = kg; k < K; k += 4) {
          const float e = staged ? sl[k * EV + lane] : expf(ap[(long)k * plane] / w - mx);
          pp[(long)k * n] = e / S;
        }
    }
    __syncthreads();                                      // the reduction rows are reused by the next slab
  }
}

inline int grid_for(long n) {
  long nb = (n + 255) / 256;
  if (nb > 65536) nb = 65536;
  return nb < 1 ? 1 : (int)nb;
}

}  // namespace

extern "C" {

int am_seg_gather(const float* vol, int X, int Y, int Z, int o0, int o1, int o2, int T0, int T1, int T2, int axes, float* out, void* stream) {
  if (!vol || !out || X <= 0 || Y <= 0 || Z <= 0 || T0 <= 0 || T1 <= 0 || T2 <= 0 || axes < 0 || axes > 7) return -2;
  const int M = 1 << __builtin_popcount(axes);
  AM_LAUNCH(seg_gather_kernel, dim3(grid_for((long)T0 * T1 * T2 * M)), dim3(256), 0, (hipStream_t)stream, vol, X, Y, Z, o0, o1, o2, T0, T1,
            T2, axes, M, out);
  AM_CHECK_LAUNCH();
  return 0;
}

int am_seg_upcat(int dtype, const void* u, const void* skip, void* y, int B, int D, int H, int W, int C, int factor, void* stream) {
  if (!u || !skip || !y || B <= 0 || C <= 0 || C % 8 || (factor != 1 && factor != 2)) return -2;
  if (D <= 0 || H <= 0 || W <= 0 || D % factor || H % factor || W % factor) return -2;
  if (((uintptr_t)u | (uintptr_t)skip | (uintptr_t)y) & 15) return -3;
  const long nvox = (long)B * D * H * W;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == AM_DT_F32) {
    AM_LAUNCH(seg_upcat_kernel<float>, dim3(grid_for(nvox * 2 * (C / 4))), dim3(256), 0, st, (const float*)u, (const float*)skip, (float*)y, B,
              D, H, W, C, factor);
  } else if (dtype == AM_DT_BF16) {
    AM_LAUNCH(seg_upcat_kernel<bf16_t>, dim3(grid_for(nvox * 2 * (C / 8))), dim3(256), 0, st, (const bf16_t*)u, (const bf16_t*)skip,
              (bf16_t*)y, B, D, H, W, C, factor);
  } else {
    return -2;
  }
  AM_CHECK_LAUNCH();
  return 0;
}

static int seg_head_launch(int dtype, const HeadArgs& a, void* stream) {
  if (!a.f || !a.w || !a.bias || a.B <= 0 || a.T0 <= 0 || a.T1 <= 0 || a.T2 <= 0 || a.C <= 0 || a.K <= 0) return -2;
  if (a.acc && a.C > AM_SEG_LDS_C) return -2;
  const long nt = (long)a.T0 * a.T1 * a.T2;
  const long tiles = (nt + HV - 1) / HV * (a.acc ? 1 : a.B);
  if (tiles > 0x7fffffffL) return -2;
  const size_t lds = a.C <= AM_SEG_LDS_C ? (size_t)HV * (a.C + 1) * sizeof(float) : 0;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == AM_DT_F32) AM_LAUNCH(seg_head_kernel<float>, dim3((unsigned)tiles), dim3(256), lds, st, a);
  else if (dtype == AM_DT_BF16) AM_LAUNCH(seg_head_kernel<bf16_t>, dim3((unsigned)tiles), dim3(256), lds, st, a);
  else return -2;
  AM_CHECK_LAUNCH();
  return 0;
}

int am_seg_head(int dtype, const void* f, int B, int D, int H, int W, int C, const float* w, const float* bias, int K, float* logits,
                void* stream) {
  if (!logits) return -2;
  HeadArgs a{};
  a.f = f; a.B = B; a.T0 = D; a.T1 = H; a.T2 = W; a.C = C; a.w = w; a.bias = bias; a.K = K; a.logits = logits;
  return seg_head_launch(dtype, a, stream);
}

int am_seg_head_accumulate(int dtype, const void* f, int axes, int T0, int T1, int T2, int C, const float* w, const float* bias, int K,
                           const float* gauss, float* acc, float* wsum, int X, int Y, int Z, int s0, int s1, int s2, void* stream) {
  if (!acc || !wsum || axes < 0 || axes > 7) return -2;
  if (s0 < 0 || s1 < 0 || s2 < 0 || s0 + T0 > X || s1 + T1 > Y || s2 + T2 > Z) return -2;    // the tile lies inside the padded volume
  HeadArgs a{};
  a.f = f; a.B = 1 << __builtin_popcount(axes); a.T0 = T0; a.T1 = T1; a.T2 = T2; a.C = C; a.w = w; a.bias = bias; a.K = K;
  a.axes = axes; a.gauss = gauss; a.acc = acc; a.wsum = wsum; a.X = X; a.Y = Y; a.Z = Z; a.s0 = s0; a.s1 = s1; a.s2 = s2;
  return seg_head_launch(dtype, a, stream);
}

int am_seg_finalize(const float* acc, const float* wsum, int K, int Xp, int Yp, int Zp, int c0, int c1, int c2, int X, int Y, int Z,
                    float* logits, void* labels, int label_bytes, void* stream) {
  if (!acc || !wsum || K <= 0 || X <= 0 || Y <= 0 || Z <= 0 || c0 < 0 || c1 < 0 || c2 < 0) return -2;
  if (c0 + X > Xp || c1 + Y > Yp || c2 + Z > Zp) return -2;
  if (!logits && !labels) return -2;
  if (labels && !((label_bytes == 1 && K <= 255) || (label_bytes == 2 && K <= 32767))) return -2;
  const long n = (long)X * Y * Z;
  hipStream_t st = (hipStream_t)stream;
  if (labels && label_bytes == 2)
    AM_LAUNCH(seg_finalize_kernel<int16_t>, dim3(grid_for(n)), dim3(256), 0, st, acc, wsum, K, Xp, Yp, Zp, c0, c1, c2, X, Y, Z, logits,
              (int16_t*)labels);
  else
    AM_LAUNCH(seg_finalize_kernel<uint8_t>, dim3(grid_for(n)), dim3(256), 0, st, acc, wsum, K, Xp, Yp, Zp, c0, c1, c2, X, Y, Z, logits,
              (uint8_t*)labels);
  AM_CHECK_LAUNCH();
  return 0;
}

int am_seg_export(const float* acc, const float* wsum, int K, int Xp, int Yp, int Zp, int c0, int c1, int c2, int X, int Y, int Z, int nonlin,
                  const int32_t* region_order, float* probs, void* labels, int label_bytes, void* stream) {
  if (!acc || !wsum || K <= 0 || X <= 0 || Y <= 0 || Z <= 0 || c0 < 0 || c1 < 0 || c2 < 0) return -2;
  if (c0 + X > Xp || c1 + Y > Yp || c2 + Z > Zp) return -2;
  if (!probs && !labels) return -2;
  if (nonlin == AM_SEG_SOFTMAX ? region_order != nullptr : (nonlin != AM_SEG_SIGMOID || !region_order)) return -2;
  if (labels && label_bytes != 1 && label_bytes != 2) return -2;
  if (labels && nonlin == AM_SEG_SOFTMAX && K - 1 > (label_bytes == 1 ? 255 : 32767)) return -2;
  ExportArgs a{acc, wsum, K, Xp, Yp, Zp, c0, c1, c2, X, Y, Z, nonlin, region_order, probs, labels, 0};
  a.staged = nonlin == AM_SEG_SOFTMAX && probs && K <= EXPORT_LDS_K;
  const size_t lds = (size_t)(8 + (a.staged ? K : 0)) * EV * sizeof(float);
  long slabs = ((long)X * Y * Z + EV - 1) / EV;
  if (slabs > 65536) slabs = 65536;
  hipStream_t st = (hipStream_t)stream;
  AM_HIP((am_lds_optin<seg_export_kernel<uint8_t>, seg_export_kernel<int16_t>>()));
  if (labels && label_bytes == 2) AM_LAUNCH(seg_export_kernel<int16_t>, dim3((unsigned)slabs), dim3(256), lds, st, a);
  else AM_LAUNCH(seg_export_kernel<uint8_t>, dim3((unsigned)slabs), dim3(256), lds, st, a);
  AM_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
