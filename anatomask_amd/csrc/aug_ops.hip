// Device-side spatial augmentation of the data feed (gfx950, VALU / HBM bound): what batchgenerators' SpatialTransform + MirrorTransform
// do on the host in the reference's worker processes (P/pretrain_AntoMask.py:57-150: rotation +-30 deg and isotropic scaling 0.7-1.4,
// p = 0.2 each, order-3 spline interpolation of the data, constant border 0; then mirroring of every axis with p = 0.5), applied to
// the ENLARGED patch the loader crops (nnunetv2/training/data_augmentation/compute_initial_patch_size.py:4-24):
//   am_spline_prefilter   cubic B-spline coefficients of a volume, in place, separable IIR with mirror boundaries -- exactly
//                         scipy.ndimage.spline_filter(order=3, mode='mirror'), which is what map_coordinates(order=3, mode='constant')
//                         applies before interpolating (batchgenerators.augmentations.utils.interpolate_img calls map_coordinates)
//   am_resample_affine    out[o] = interp(src, A * (o, 1)): per-sample 3x4 affine (rotation, scale, centring, mirror flips folded
//                         in); order 0 = nearest voxel, floor(x + 0.5) (integer crop / flip when A is one), 1 = trilinear, 3 = cubic
//                         B-spline over prefiltered coefficients; every order with scipy's map_coordinates(mode='constant') rules:
//                         a coordinate outside [0, n-1] on any axis -> cval (order 0 too: -0.3 is outside although it rounds to 0),
//                         mirrored coefficient access at the edges.  Null pointers / non-positive extents / other orders: -2, no launch
//   am_resample_labels    the segmentation half of the same SpatialTransform (border_mode_seg 'constant', border_cval_seg -1, order_seg 1,
//                         P/pretrain_AntoMask.py:80-91) at the SAME coordinates: int16 labels by batchgenerators' per-label vote
//                         (interpolate_img(is_seg=True)), then RemoveLabelTransform(-1, 0) (:118) and, optionally,
//                         ConvertSegmentationToRegionsTransform (:139-143) as one uint8 plane per region, in the same pass
#include "common.h"
#include "../../include/anatomask_hip.h"

namespace {

// one thread per line along `axis`; lines are enumerated so that consecutive threads take consecutive innermost positions
// (axis 0 / 1: coalesced across the wave; axis 2: each thread walks its own contiguous line, served by L2)
__global__ __launch_bounds__(256) void spline_prefilter_kernel(float* __restrict__ v, int D, int H, int W, int axis) {
  const long nline = axis == 0 ? (long)H * W : axis == 1 ? (long)D * W : (long)D * H;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= nline) return;
  const int n = axis == 0 ? D : axis == 1 ? H : W;
  long base, stride;
  if (axis == 0) { base = t; stride = (long)H * W; }
  else if (axis == 1) { base = (t / W) * (long)H * W + t % W; stride = W; }
  else { base = t * (long)W; stride = 1; }
  if (n < 2) return;
  const double z = -0.26794919243112270647;                  // sqrt(3) - 2
  const float zf = (float)z, lambda = (float)((1.0 - z) * (1.0 - 1.0 / z));
  float* p = v + base;
  // causal initialisation for a mirror boundary (exact sum over the 2n - 2 periodic samples; terms vanish below fp32 after ~24)
  double zi = z, c0 = (double)p[0] * lambda;
  const int m = n < 40 ? n : 40;
  for (int i = 1; i < m; ++i) { c0 += zi * (double)p[i * stride] * lambda; zi *= z; }
  if (m == n) {
    for (int i = n - 2; i > 0; --i) { c0 += zi * (double)p[i * stride] * lambda; zi *= z; }
    c0 /= (1.0 - zi);
  }
  float prev = (float)c0;
  p[0] = prev;
  for (int i = 1; i < n; ++i) { prev = p[i * stride] * lambda + zf * prev; p[i * stride] = prev; }
  prev = (float)((z / (z * z - 1.0)) * ((double)p[(n - 1) * stride] + z * (double)p[(n - 2) * stride]));
  p[(n - 1) * stride] = prev;
  for (int i = n - 2; i >= 0; --i) { prev = zf * (prev - p[i * stride]); p[i * stride] = prev; }
}

__device__ __forceinline__ int mirror_idx(int i, int n) {
  i = i < 0 ? -i : i;
  i = i > n - 1 ? 2 * (n - 1) - i : i;
  return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}
__device__ __forceinline__ void bspline_w(float f, float* w) {   // weights of the 4 coefficients around floor(x), f = x - floor(x)
  const float f2 = f * f, f3 = f2 * f, g = 1.f - f;
  w[0] = g * g * g * (1.f / 6.f);
  w[1] = 2.f / 3.f - f2 + 0.5f * f3;
  w[2] = 2.f / 3.f - g * g + 0.5f * g * g * g;
  w[3] = f3 * (1.f / 6.f);
}

struct Aff { float a[12]; };

// source coordinate A (d, h, w, 1) of an output voxel: ONE definition for the image and the label kernel, so that a label and its image
// voxel sample the same fp32 point.  Which products of a0 d + a1 h + a2 w + a3 are fused into the following sum is the compiler's choice
// per kernel when contraction is on, so it is switched off here and the operations are spelled out -- the ones resample_affine_kernel
// has always compiled to (its results stay bit for bit what they were).
__device__ __forceinline__ void source_coord(const Aff& A, int d, int h, int w, float& pz, float& py, float& px) {
#pragma clang fp contract(off)
  const float fd = (float)d, fh = (float)h, fw = (float)w;
  pz = (__builtin_fmaf(A.a[0], fd, A.a[1] * fh) + A.a[2] * fw) + A.a[3];
  py = __builtin_fmaf(A.a[6], fw, __builtin_fmaf(A.a[5], fh, A.a[4] * fd)) + A.a[7];
  px = __builtin_fmaf(A.a[10], fw, __builtin_fmaf(A.a[8], fd, A.a[9] * fh)) + A.a[11];
}

__global__ __launch_bounds__(256) void resample_affine_kernel(const float* __restrict__ src, int Ds, int Hs, int Ws, float* __restrict__ dst,
                                                              int D, int H, int W, Aff A, int order, float cval) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)D * H * W) return;
  const int w = (int)(i % W), h = (int)((i / W) % H), d = (int)(i / ((long)W * H));
  float pz, py, px;
  source_coord(A, d, h, w, pz, py, px);
  float out = cval;
  if (pz >= 0.f && pz <= Ds - 1.f && py >= 0.f && py <= Hs - 1.f && px >= 0.f && px <= Ws - 1.f) {   // scipy: outside [0, n-1] -> cval, every order
    const int bz = (int)floorf(pz), by = (int)floorf(py), bx = (int)floorf(px);
    if (order == 0) {                                              // nearest: floor(p + 0.5), ties upwards
      const int iz = min((int)floorf(pz + 0.5f), Ds - 1), iy = min((int)floorf(py + 0.5f), Hs - 1), ix = min((int)floorf(px + 0.5f), Ws - 1);
      out = src[((long)iz * Hs + iy) * Ws + ix];
    } else if (order == 1) {
      const float fz = pz - bz, fy = py - by, fx = px - bx;
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int iz = min(bz + (k >> 2), Ds - 1), iy = min(by + ((k >> 1) & 1), Hs - 1), ix = min(bx + (k & 1), Ws - 1);
        const float wt = ((k >> 2) ? fz : 1.f - fz) * (((k >> 1) & 1) ? fy : 1.f - fy) * ((k & 1) ? fx : 1.f - fx);
        s += wt * src[((long)iz * Hs + iy) * Ws + ix];
      }
      out = s;
    } else {
      float wz[4], wy[4], wx[4];
      bspline_w(pz - bz, wz); bspline_w(py - by, wy); bspline_w(px - bx, wx);
      int ix[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) ix[c] = mirror_idx(bx - 1 + c, Ws);
      float s = 0.f;
#pragma unroll
      for (int a_ = 0; a_ < 4; ++a_) {
        const long zo = (long)mirror_idx(bz - 1 + a_, Ds) * Hs;
#pragma unroll
        for (int b_ = 0; b_ < 4; ++b_) {
          const float* row = src + (zo + mirror_idx(by - 1 + b_, Hs)) * Ws;
          const float r = wx[0] * row[ix[0]] + wx[1] * row[ix[1]] + wx[2] * row[ix[2]] + wx[3] * row[ix[3]];
          s += wz[a_] * wy[b_] * r;
        }
      }
      out = s;
    }
  }
  dst[i] = out;
}

// label of one output voxel, before the removal: batchgenerators' interpolate_img(is_seg=True) at the point source_coord gives.
// order 0: the label at floor(p + 0.5), outside -> cval (the rule of resample_affine_kernel).  order 1: per label c the mask (seg == c)
// is interpolated trilinearly and the LARGEST c with a value >= 0.5 wins, 0 when none does; every mask is -1 outside, so outside -> 0.
// The masks' values are the sums of the corner weights per label: 8 gathered labels compared with one another, no loop over labels.
__device__ __forceinline__ int resample_label(const int16_t* __restrict__ src, int Ds, int Hs, int Ws, const Aff& A, int d, int h, int w,
                                              int order, int cval) {
  float pz, py, px;
  source_coord(A, d, h, w, pz, py, px);
  if (!(pz >= 0.f && pz <= Ds - 1.f && py >= 0.f && py <= Hs - 1.f && px >= 0.f && px <= Ws - 1.f)) return order == 0 ? cval : 0;
  if (order == 0) {
    const int iz = min((int)floorf(pz + 0.5f), Ds - 1), iy = min((int)floorf(py + 0.5f), Hs - 1), ix = min((int)floorf(px + 0.5f), Ws - 1);
    return src[((long)iz * Hs + iy) * Ws + ix];
  }
  const int bz = (int)floorf(pz), by = (int)floorf(py), bx = (int)floorf(px);
  const float fz = pz - bz, fy = py - by, fx = px - bx;
  int lab[8];
  float wt[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int iz = min(bz + (k >> 2), Ds - 1), iy = min(by + ((k >> 1) & 1), Hs - 1), ix = min(bx + (k & 1), Ws - 1);
    wt[k] = ((k >> 2) ? fz : 1.f - fz) * (((k >> 1) & 1) ? fy : 1.f - fy) * ((k & 1) ? fx : 1.f - fx);
    lab[k] = src[((long)iz * Hs + iy) * Ws + ix];
  }
  const int none = -0x7fffffff - 1;                                 // below every int16 label
  int best = none;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += lab[j] == lab[k] ? wt[j] : 0.f;   // corner order 0..7
    best = s >= 0.5f ? max(best, lab[k]) : best;
  }
  return best == none ? 0 : best;
}

// One output voxel per lane, as in resample_affine_kernel: consecutive lanes gather neighbouring source voxels, and the 2-byte label
// stores and 1-byte region stores of a wave are contiguous.  (A lane owning 4 consecutive voxels, so that labels and regions leave as
// 8- and 4-byte stores, was built and measured: 1.39 x slower on 205^3 -> 128^3, because each gather instruction of a wave then spans
// four times the source range; the narrow stores cost nothing measurable.  DESIGN.md section 6.)
__global__ __launch_bounds__(256) void resample_labels_kernel(const int16_t* __restrict__ src, int Ds, int Hs, int Ws, int16_t* __restrict__ dst,
                                                              int D, int H, int W, Aff A, int order, int cval, int remove_from, int remove_to,
                                                              const int32_t* __restrict__ region_bits, int n_lut, int n_regions,
                                                              uint8_t* __restrict__ regions_out) {
  const long n = (long)D * H * W;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int w = (int)(i % W), h = (int)((i / W) % H), d = (int)(i / ((long)W * H));
  int l = resample_label(src, Ds, Hs, Ws, A, d, h, w, order, cval);
  l = l == remove_from ? remove_to : l;
  if (dst) dst[i] = (int16_t)l;
  if (regions_out) {
    const unsigned bits = l >= 0 && l < n_lut ? (unsigned)region_bits[l] : 0u;
    for (int r = 0; r < n_regions; ++r) regions_out[(long)r * n + i] = (uint8_t)((bits >> r) & 1u);
  }
}

}  // namespace

extern "C" {

int am_spline_prefilter(float* vol, int D, int H, int W, void* stream) {
  if (!vol || D < 1 || H < 1 || W < 1) return -1;
  hipStream_t st = (hipStream_t)stream;
  for (int axis = 0; axis < 3; ++axis) {
    const long nline = axis == 0 ? (long)H * W : axis == 1 ? (long)D * W : (long)D * H;
    AM_LAUNCH(spline_prefilter_kernel, dim3((unsigned)((nline + 255) / 256)), dim3(256), 0, st, vol, D, H, W, axis);
    AM_CHECK_LAUNCH();
  }
  return 0;
}

int am_resample_affine(const float* src, int Ds, int Hs, int Ws, float* dst, int D, int H, int W, const float* affine_host12, int order,
                       float cval, void* stream) {
  if (order != 0 && order != 1 && order != 3) return -2;
  if (!src || !dst || !affine_host12 || Ds <= 0 || Hs <= 0 || Ws <= 0 || D <= 0 || H <= 0 || W <= 0) return -2;
  Aff A;
  for (int i = 0; i < 12; ++i) A.a[i] = affine_host12[i];
  const long n = (long)D * H * W;
  AM_LAUNCH(resample_affine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, Ds, Hs, Ws, dst, D, H, W, A,
            order, cval);
  AM_CHECK_LAUNCH();
  return 0;
}

int am_resample_labels(const int16_t* src, int Ds, int Hs, int Ws, int16_t* dst, int D, int H, int W, const float* affine_host12, int order,
                       int cval, int remove_from, int remove_to, const int32_t* region_bits, int n_lut, int n_regions, uint8_t* regions_out,
                       void* stream) {
  if (order != 0 && order != 1) return -2;
  if (!src || !affine_host12 || (!dst && !regions_out) || Ds <= 0 || Hs <= 0 || Ws <= 0 || D <= 0 || H <= 0 || W <= 0) return -2;
  if (regions_out && (!region_bits || n_regions < 1 || n_regions > 32)) return -2;
  Aff A;
  for (int i = 0; i < 12; ++i) A.a[i] = affine_host12[i];
  const long n = (long)D * H * W;
  AM_LAUNCH(resample_labels_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, Ds, Hs, Ws, dst, D, H, W, A,
            order, cval, remove_from, remove_to, region_bits, n_lut, n_regions, regions_out);
  AM_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
