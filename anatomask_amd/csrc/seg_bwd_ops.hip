// STUNet segmentation fine-tuning (gfx950): the backward of the two layers of the segmentation network that are neither convolutions nor
// norms (seg_ops.hip has their forwards).
//   seg_head_bwd    backward of the 1x1 head C -> K in ONE pass over the class-major logit gradient: df = W^T dl (compute dtype, rounded
//                   once, optionally added to what df holds), dw += dl f^T, db += sum dl.  Both contractions run from the same staged
//                   [K][64-voxel] tile of dl on the exact fp32 matrix instruction (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain).
//                   dw / db: per-workgroup partial sums in a caller-supplied workspace (a persistent grid of at most
//                   AM_SEG_HEAD_BWD_SLOTS workgroups, each the only writer of its slot), then an ordered fold -- no atomics, the same
//                   input gives the same bits.
//   seg_upcat_bwd   backward of cat(nearest_up(u), skip): du = fp32 sum of the f^3 fine voxels of the first C channels (rounded once),
//                   dskip = the second C channels; 16-byte chunks.
#include "common.h"
#include "../../include/anatomask_hip.h"

namespace {

constexpr int BV = AM_SEG_HEAD_BWD_TILE;                  // voxels per staged tile
constexpr int VP = BV + 1;                                // row pitch of the staged dl tile (floats)
constexpr int KCHUNK = 256;                               // classes per launch (the staged tile holds all of them)
constexpr int DWREG = 4;                                  // dw output tiles a wave keeps in registers
constexpr size_t LDS_MAX = 150 * 1024, LDS_SMALL = 64 * 1024;

// row pitch (floats) of a [rows][C] LDS image read as 4 rows x 16 consecutive channels per wave: pitch = 16 (mod 32) keeps the two
// rows of a 32-lane half on disjoint banks
inline __host__ __device__ int pitch16(int C) { return C + (48 - C % 32) % 32; }

struct HeadBwdArgs {
  const float* dl; long dl_bstride;                       // [B][K of this chunk][nt], batch stride in floats (the FULL K x nt)
  const void* f; const float* w; void* df; float* ws;     // f, df [B][nt][C]; w [K][C]; ws [gridDim.x][K C + K]
  int C, K; long nt, tiles_per_b, tiles;
  int accumulate, fstaged, wstaged, dwreg, dl_vec4;
};

template <typename T> __device__ __forceinline__ void add_store4(T* p, const f32x4& v, bool accumulate);
template <> __device__ __forceinline__ void add_store4<float>(float* p, const f32x4& v, bool accumulate) {
  f32x4 o = v;
  if (accumulate) o += *(const f32x4*)p;
  *(f32x4*)p = o;
}
template <> __device__ __forceinline__ void add_store4<bf16_t>(bf16_t* p, const f32x4& v, bool accumulate) {
  typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
  f32x4 o = v;
  if (accumulate) {
    const u32x2 old = *(const u32x2*)p;
    o[0] += __uint_as_float(old[0] << 16); o[1] += __uint_as_float(old[0] & 0xffff0000u);
    o[2] += __uint_as_float(old[1] << 16); o[3] += __uint_as_float(old[1] & 0xffff0000u);
  }
  u32x2 n;
  n[0] = (uint32_t)f2bf(o[0]) | ((uint32_t)f2bf(o[1]) << 16);
  n[1] = (uint32_t)f2bf(o[2]) | ((uint32_t)f2bf(o[3]) << 16);
  *(u32x2*)p = n;
}

// One workgroup = 4 waves; tile t = blockIdx.x, blockIdx.x + gridDim.x, ... (64 consecutive voxels of one sample).  Per tile:
//   stage dl [K16][64] (rows >= K and voxels past the sample: zeros) and, where they fit, f [64][C] and (once) w [K4][C] as fp32 in LDS;
//   db: 4 threads per class sum 16 voxels each, combined in a fixed order;
//   dw: 16 x 16 (class x channel) output tiles, tile i on wave i % 4 -- D[k][c] = sum_v dl[k][v] f[v][c], 16 matrix instructions of 4
//       voxels each, on top of the wave's own partial sums: in registers over all of the workgroup's tiles where a wave owns at most
//       DWREG output tiles (written to the slot once, at the end), else in the slot (the same lane owns the same elements in every tile);
//   df: wave j owns voxels 16 j .. 16 j + 15 -- D[c][v] = sum_k w[k][c] dl[k][v] per 16-channel tile, K4 / 4 matrix instructions; a lane
//       ends up with 4 consecutive channels of one voxel: one 8- / 16-byte (read-add-)store.
template <typename T>
__global__ __launch_bounds__(256) void seg_head_bwd_kernel(HeadBwdArgs a) {
  extern __shared__ float s_lds[];
  const int C = a.C, K = a.K;
  const int K16 = (K + 15) & ~15, K4 = (K + 3) & ~3, FP = pitch16(C);
  float* dl_s = s_lds;                                    // [K16][VP]
  float* f_s = dl_s + K16 * VP;                           // [BV][FP]
  float* w_s = f_s + (a.fstaged ? BV * FP : 0);           // [K4][FP]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  const long KC = (long)K * C;
  float* slot = a.ws + (long)blockIdx.x * (KC + K);
  const T* f = (const T*)a.f;
  T* df = (T*)a.df;
  const int nkt = K16 >> 4, nct = (C + 15) >> 4;
  constexpr int EPC = 16 / sizeof(T);

  if (a.wstaged)
    for (int e = tid; e < K4 * C; e += 256) {
      const int k = e / C, c = e - k * C;
      w_s[k * FP + c] = k < K ? a.w[e] : 0.f;
    }

  // load (store = false) or store the lane's 4 elements of dw output tile i in the slot: rows kb .. kb + 3 of column c
  auto slot_tile = [&](int i, f32x4 acc, bool store) {
    const int kt = i / nct, c = (i - kt * nct) * 16 + r16;
    const int kb = kt * 16 + 4 * g;
    if (c < C) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (kb + r < K) {
          if (store) slot[(long)(kb + r) * C + c] = acc[r];
          else acc[r] = slot[(long)(kb + r) * C + c];
        }
    }
    return acc;
  };
  f32x4 racc[DWREG];
#pragma unroll
  for (int j = 0; j < DWREG; ++j) racc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  bool first = true;
  for (long t = blockIdx.x; t < a.tiles; t += gridDim.x, first = false) {
    const int b = (int)(t / a.tiles_per_b);
    const long v0 = (t - (long)b * a.tiles_per_b) * BV;
    const int nv = (int)(a.nt - v0 < BV ? a.nt - v0 : BV);
    __syncthreads();                                      // the previous tile's readers are done
    const float* dlb = a.dl + (long)b * a.dl_bstride + v0;
    // the loads of a batch are issued back to back, then stored (a load-store loop would pay one memory round trip per row)
    if (a.dl_vec4) {                                      // nt % 4 == 0: 16-byte loads, 16 lanes per class row, 16 rows per pass
      const int q = (tid & 15) * 4, r0 = tid >> 4;
      for (int kb = 0; kb < K16; kb += 64) {
        f32x4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = kb + 16 * j + r0;
          v[j] = (k < K && q < nv) ? *(const f32x4*)(dlb + (long)k * a.nt + q) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = kb + 16 * j + r0;
          if (k < K16) {
            float* d = dl_s + k * VP + q;
            d[0] = v[j][0]; d[1] = v[j][1]; d[2] = v[j][2]; d[3] = v[j][3];
          }
        }
      }
    } else {
      for (int kb = 0; kb < K16; kb += 32) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = kb + 4 * j + wave;
          v[j] = (k < K && lane < nv) ? dlb[(long)k * a.nt + lane] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = kb + 4 * j + wave;
          if (k < K16) dl_s[k * VP + lane] = v[j];
        }
      }
    }
    if (a.fstaged) {
      const int cc = C / EPC;
      for (int e = tid; e < BV * cc; e += 256) {
        const int vl = e / cc, c = (e - vl * cc) * EPC;
        float v[EPC];
        if (vl < nv) {
          chunk_to_f<T>(*(const u32x4*)(f + ((long)b * a.nt + v0 + vl) * C + c), v);
        } else {
#pragma unroll
          for (int j = 0; j < EPC; ++j) v[j] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < EPC; ++j) f_s[vl * FP + c + j] = v[j];
      }
    }
    __syncthreads();

    // ---- db
    for (int i0 = 0; i0 < K * 4; i0 += 256) {
      const int i = i0 + tid, k = i >> 2, q = i & 3;
      float s = 0.f;
      if (k < K)
        for (int j = 0; j < 16; ++j) s += dl_s[k * VP + q * 16 + j];
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      if (k < K && q == 0) slot[KC + k] = first ? s : slot[KC + k] + s;
    }

    // ---- dw
    auto dw_tile = [&](int i, f32x4 acc) {                // output tile i += its 16 x 16 x 64 product of this voxel tile
      const int kt = i / nct, c = (i - kt * nct) * 16 + r16;
      const bool cok = c < C;
      const float* arow = dl_s + (kt * 16 + r16) * VP + g;
#pragma unroll 4
      for (int vs = 0; vs < BV; vs += 4) {
        const float av = arow[vs];
        float bv = 0.f;
        if (cok) {
          if (a.fstaged) bv = f_s[(vs + g) * FP + c];
          else if (vs + g < nv) bv = TT<T>::ld(f + ((long)b * a.nt + v0 + vs + g) * C + c);
        }
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
      }
      return acc;
    };
    if (a.dwreg) {                                        // at most DWREG tiles per wave: their sums stay in registers over all tiles
#pragma unroll
      for (int j = 0; j < DWREG; ++j)
        if (wave + 4 * j < nkt * nct) racc[j] = dw_tile(wave + 4 * j, racc[j]);
    } else {
      for (int i = wave; i < nkt * nct; i += 4) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (!first) acc = slot_tile(i, acc, false);
        slot_tile(i, dw_tile(i, acc), true);
      }
    }

    // ---- df
    const int vl = wave * 16 + r16;
    for (int ct = 0; ct < nct; ++ct) {
      const int c = ct * 16 + r16;
      const bool cok = c < C;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < K4; k0 += 4) {
        const int k = k0 + g;
        float av = 0.f;
        if (cok) {
          if (a.wstaged) av = w_s[k * FP + c];
          else if (k < K) av = a.w[(long)k * C + c];
        }
        const float bv = dl_s[k * VP + vl];
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
      }
      const int cb = ct * 16 + 4 * g;                     // D rows 4 g .. 4 g + 3 = channels cb .. cb + 3 of voxel vl
      if (vl < nv && cb < C) add_store4<T>(df + ((long)b * a.nt + v0 + vl) * C + cb, acc, a.accumulate != 0);
    }
  }
  if (a.dwreg) {
#pragma unroll
    for (int j = 0; j < DWREG; ++j)
      if (wave + 4 * j < nkt * nct) slot_tile(wave + 4 * j, racc[j], true);
  }
}

// dw[i] += sum over the slots, i < K C; db[i - K C] += ... for the rest: 64 outputs per workgroup, 4 contiguous quarters of the slots
// summed in order by one thread each, the quarters then added in order
__global__ __launch_bounds__(256) void seg_head_bwd_fold_kernel(const float* __restrict__ ws, int slots, long n, long KC, float* __restrict__ dw,
                                                                float* __restrict__ db) {
  __shared__ float part[4][64];
  const int o = threadIdx.x & 63, q = threadIdx.x >> 6;
  const long i = (long)blockIdx.x * 64 + o;
  float s = 0.f;
  if (i < n) {
    const int per = (slots + 3) / 4;
    const int s0 = q * per, s1 = s0 + per < slots ? s0 + per : slots;
    for (int j = s0; j < s1; ++j) s += ws[(long)j * n + i];
  }
  part[q][o] = s;
  __syncthreads();
  if (q == 0 && i < n) {
    const float tot = ((part[0][o] + part[1][o]) + part[2][o]) + part[3][o];
    if (i < KC) dw[i] += tot;
    else db[i - KC] += tot;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void seg_upcat_bwd_kernel(const T* __restrict__ dy, T* __restrict__ du, T* __restrict__ dskip, int B, int D,
                                                            int H, int W, int C, int factor) {
  constexpr int EPC = 16 / sizeof(T);
  const int cc = C / EPC;                                 // chunks per voxel of du / dskip
  const int d = D / factor, h = H / factor, w = W / factor;
  const long n = (long)B * d * h * w * cc;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long cv = i / cc;
    const int c = (int)(i - cv * cc) * EPC;
    long r = cv;
    const int iw = (int)(r % w); r /= w;
    const int ih = (int)(r % h); r /= h;
    const int id = (int)(r % d);
    const int b = (int)(r / d);
    float s[EPC];
#pragma unroll
    for (int j = 0; j < EPC; ++j) s[j] = 0.f;
    for (int z = 0; z < factor; ++z)
      for (int y = 0; y < factor; ++y)
        for (int x = 0; x < factor; ++x) {
          const long v = (((long)b * D + id * factor + z) * H + ih * factor + y) * W + iw * factor + x;
          const T* row = dy + v * 2 * C;
          float t[EPC];
          chunk_to_f<T>(*(const u32x4*)(row + c), t);
#pragma unroll
          for (int j = 0; j < EPC; ++j) s[j] += t[j];
          *(u32x4*)(dskip + v * C + c) = *(const u32x4*)(row + C + c);
        }
    *(u32x4*)(du + cv * C + c) = f_to_chunk<T>(s);
  }
}

inline int grid_for(long n) {
  long nb = (n + 255) / 256;
  if (nb > 65536) nb = 65536;
  return nb < 1 ? 1 : (int)nb;
}

}  // namespace

extern "C" {

int am_seg_head_bwd(int dtype, const float* dlogits, const void* f, const float* w, int B, int D, int H, int W, int C, int K, void* df,
                    int accumulate, float* dw, float* db, float* workspace, long workspace_floats, void* stream) {
  if (!dlogits || !f || !w || !df || !dw || !db || !workspace) return -2;
  if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 || K <= 0) return -2;
  if (dtype != AM_DT_F32 && dtype != AM_DT_BF16) return -2;
  if (((uintptr_t)f | (uintptr_t)df) & 15) return -3;
  const long nt = (long)D * H * W;
  const long tiles_per_b = (nt + BV - 1) / BV, tiles = tiles_per_b * B;
  const int slots = (int)(tiles < AM_SEG_HEAD_BWD_SLOTS ? tiles : AM_SEG_HEAD_BWD_SLOTS);
  const int kmax = K < KCHUNK ? K : KCHUNK;
  if (workspace_floats < (long)slots * ((long)kmax * C + kmax)) return -2;
  hipStream_t st = (hipStream_t)stream;
  AM_HIP((am_lds_optin<seg_head_bwd_kernel<float>, seg_head_bwd_kernel<bf16_t>>()));
  for (int k0 = 0; k0 < K; k0 += KCHUNK) {                // (K > 256: chunks of classes; df is then rounded once per chunk)
    const int kn = K - k0 < KCHUNK ? K - k0 : KCHUNK;
    HeadBwdArgs a{};
    a.dl = dlogits + (long)k0 * nt; a.dl_bstride = (long)K * nt;
    a.f = f; a.w = w + (long)k0 * C; a.df = df; a.ws = workspace;
    a.C = C; a.K = kn; a.nt = nt; a.tiles_per_b = tiles_per_b; a.tiles = tiles;
    a.accumulate = (accumulate || k0 > 0) ? 1 : 0;
    const int K16 = (kn + 15) & ~15, K4 = (kn + 3) & ~3, FP = pitch16(C);
    size_t lds = (size_t)K16 * VP * sizeof(float);
    const size_t fl = (size_t)BV * FP * sizeof(float), wl = (size_t)K4 * FP * sizeof(float);
    if (C <= AM_SEG_LDS_C && lds + fl <= LDS_MAX) { a.fstaged = 1; lds += fl; }
    if (a.fstaged && lds + wl <= LDS_SMALL) { a.wstaged = 1; lds += wl; }
    a.dwreg = (K16 / 16) * ((C + 15) / 16) <= 4 * DWREG;
    a.dl_vec4 = nt % 4 == 0 && ((uintptr_t)dlogits & 15) == 0;
    if (dtype == AM_DT_F32) AM_LAUNCH(seg_head_bwd_kernel<float>, dim3((unsigned)slots), dim3(256), lds, st, a);
    else AM_LAUNCH(seg_head_bwd_kernel<bf16_t>, dim3((unsigned)slots), dim3(256), lds, st, a);
    AM_CHECK_LAUNCH();
    const long n = (long)kn * C + kn;
    AM_LAUNCH(seg_head_bwd_fold_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, st, (const float*)workspace, slots, n, (long)kn * C,
              dw + (long)k0 * C, db + k0);
    AM_CHECK_LAUNCH();
  }
  return 0;
}

int am_seg_upcat_bwd(int dtype, const void* dy, void* du, void* dskip, int B, int D, int H, int W, int C, int factor, void* stream) {
  if (!dy || !du || !dskip || B <= 0 || C <= 0 || C % 8 || (factor != 1 && factor != 2)) return -2;
  if (D <= 0 || H <= 0 || W <= 0 || D % factor || H % factor || W % factor) return -2;
  if (((uintptr_t)dy | (uintptr_t)du | (uintptr_t)dskip) & 15) return -3;
  const long ncoarse = (long)B * (D / factor) * (H / factor) * (W / factor);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == AM_DT_F32) {
    AM_LAUNCH(seg_upcat_bwd_kernel<float>, dim3(grid_for(ncoarse * (C / 4))), dim3(256), 0, st, (const float*)dy, (float*)du, (float*)dskip, B, D,
              H, W, C, factor);
  } else if (dtype == AM_DT_BF16) {
    AM_LAUNCH(seg_upcat_bwd_kernel<bf16_t>, dim3(grid_for(ncoarse * (C / 8))), dim3(256), 0, st, (const bf16_t*)dy, (bf16_t*)du, (bf16_t*)dskip,
              B, D, H, W, C, factor);
  } else {
    return -2;
  }
  AM_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
