// libflairhip: calibrated class thresholds (include/flairhip_calib.h).
//
//   * ffa_calib_hist: per-class histograms of the score bytes over a validation batch, split by whether the pixel's
//     target is the class -- what a threshold sweep needs, in one pass over the logits
//   * ffa_predict_thresholded_u8 / ffa_tta_predict_thresholded_u8: the label and confidence outputs of
//     ffa_predict_u8 / ffa_tta_predict_u8 under K per-class thresholds, in the one pass those make
// The reference carries a per-model threshold file through its interface (main.py --threshold_file_path,
// utils/s3.py best_thresholds.yaml, flair_zonal_detection/inference.py model_threshold_filepath) and never reads it.
//
// Definitions (the contract).
//
// Score byte.  For a pixel with logits z[0..K): m = maximum, e_k = expf(z_k - m), se = sum of e_k in class order,
// q_k = (uint8) rintf(e_k / se * 255.f).  This is class_prob_crop_kernel's arithmetic (resample_loss.hip), operation
// for operation, so q_k is bit for bit the byte ffa_predict_u8 mode 1 writes for class k at that pixel.
//
// Score histograms.  hist[k][s][q], int64 [K][2][256], accumulating like confmat: for every pixel with target t < K
// and every class k, hist[k][t == k ? 1 : 0][q_k] += 1.  A pixel with t >= K contributes nowhere (ffa_eval_stats'
// rule).  Counts are integers: equal inputs give equal bytes in any schedule.
//
// Thresholded label.  Given thr[0..K) (uint8) and fallback (uint8): class k passes when q_k >= thr[k]; the label is
// the passing class with the greatest z_k, the lowest index on a tie (the strict '>' of mode 0, restricted to passing
// classes); fallback if no class passes.  With all thresholds 0 the label plane equals mode 0 byte for byte.
//
// Confidence plane (mode 2 analogue).  q of the chosen class; 0 where the label is fallback because nothing passed.
//
// TTA path.  On an accumulator, p_k = acc_k / views, q_k = rintf(p_k * 255.f), ordering on p_k (tta_finish_kernel's
// arithmetic).
//
// ffa_calib_hist.  The thread <-> pixel walk, the grid cap and the staging of the logits through LDS in memory order
// are eval_stats_kernel's (a thread that owns a 64-byte pixel otherwise touches 32 cache lines per wave instruction).
// The block keeps a private histogram in LDS (32-bit integer atomics) and flushes its non-empty bins with 64-bit
// integer atomics at the end: confmat's pattern.  K * 2 * 256 * 4 B is 38 KB at K = 19 and 64 KB at K = 32, so the
// block's LDS is dynamic: the staging tile at the pitch in use, then the bins of KC classes, 64 KB at the most
// together.  Where K classes do not fit (bf16: K > 22 at pitch 32; f32: K > 14 at pitch 32, > 18 at pitch 24) the
// block walks its tiles once per chunk of KC classes.  19 classes in bf16 take 58 KB: two blocks per CU, one pass.
// A trained model puts most q_k at 0 and the winner near 255: 64 lanes of a wave would queue on one LDS address, K
// times per pixel.  Bins 0 and 255 therefore never go through per-lane atomics: a lane counts them in registers (per
// class one word of four 8-bit fields, q 0 / q 255 by side), and every 255 tiles and at the end the fields are summed
// over the wave and added with one LDS atomic per wave, class and field.  Only the scores 1..254 take per-lane atomics.
// Measured at 32 x 512 x 512 x 19, pitch 32, bf16: 360 us on saturated logits against 464 us for
// ballot + popcount per class and tile and 618 us for per-lane atomics throughout; on N(0, 2^2) logits 378 / 474 / 305.
#include "ffa_common.h"

#define FFA_CALIB_THREADS 256
#define FFA_CALIB_BLOCKS 1024   // grid cap: a block walks tiles blockIdx.x, + gridDim.x, ...
#define FFA_CALIB_LDS 65536     // the block's LDS budget: what a launch gets without asking for more
#define FFA_CALIB_BINS 512      // per class: 2 sides x 256 scores

// KR: the class count rounded up to a multiple of 8 (sizes the register arrays); KC: classes per chunk
template <typename T, int KR>
__global__ void __launch_bounds__(FFA_CALIB_THREADS)
calib_hist_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ tgt, unsigned long long* __restrict__ out,
                  long long npix, int K, int Cp, int KC) {
  constexpr int EPP = 16 / (int)sizeof(T);  // elements per 16-byte piece
  constexpr int MAXP = FFA_CE_MAXK / EPP;   // pieces per pixel at the largest pitch: 4 (bf16) / 8 (f32)
  extern __shared__ __align__(16) unsigned char calib_lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int np = Cp / EPP;   // pieces per pixel
  const int slots = np | 1;  // LDS pitch of a pixel in 16-byte slots: odd
  unsigned char* tile = calib_lds;
  unsigned int* hist = reinterpret_cast<unsigned int*>(calib_lds + FFA_CALIB_THREADS * slots * 16);  // [KC][2][256]
  const long long ntiles = (npix + FFA_CALIB_THREADS - 1) / FFA_CALIB_THREADS;
  int loff[MAXP];  // LDS byte offset of piece tid + 256 k of a tile
#pragma unroll
  for (int k = 0; k < MAXP; ++k) {
    const int idx = tid + FFA_CALIB_THREADS * k;
    loff[k] = ((idx / np) * slots + idx % np) * 16;
  }
  uint4 pre[MAXP];
  auto gload = [&](long long ti) {
    const long long base = ti * FFA_CALIB_THREADS;
    const long long left = npix - base;
    const int npc = (int)(left < FFA_CALIB_THREADS ? left : FFA_CALIB_THREADS) * np;
    const uint4* src = reinterpret_cast<const uint4*>(logits + base * Cp);
#pragma unroll
    for (int k = 0; k < MAXP; ++k) {
      const int idx = tid + FFA_CALIB_THREADS * k;
      if (k < np) pre[k] = idx < npc ? src[idx] : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  for (int c0 = 0; c0 < K; c0 += KC) {
    const int c1 = c0 + KC < K ? c0 + KC : K;
    const int bins = (c1 - c0) * FFA_CALIB_BINS;
    for (int i = tid; i < bins; i += FFA_CALIB_THREADS) hist[i] = 0u;
    // this lane's counts of the hot bins, per class four 8-bit fields: (q 0, rest), (q 0, class), (q 255, rest),
    // (q 255, class).  A lane adds at most one per tile, so the fields are summed over the wave and emptied every 255
    // tiles and at the end: 16-bit fields hold a wave's sum of 64 x 255.
    unsigned int cnt[KR];
#pragma unroll
    for (int k = 0; k < KR; ++k) cnt[k] = 0u;
    int since = 0;
    auto drain = [&]() {
#pragma unroll
      for (int k = 0; k < KR; ++k) {
        if (k >= c0 && k < c1) {
          unsigned int lo = cnt[k] & 0x00ff00ffu, hi = (cnt[k] >> 8) & 0x00ff00ffu;  // fields 0, 2 and 1, 3
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            lo += __shfl_xor(lo, o, 64);
            hi += __shfl_xor(hi, o, 64);
          }
          if (lane < 4) {  // lane 0: (q 0, rest), 1: (q 0, class), 2: (q 255, rest), 3: (q 255, class)
            const unsigned int w = (lane & 1) ? hi : lo;
            const unsigned int c = (lane >> 1) ? w >> 16 : w & 0xffffu;
            if (c) atomicAdd(&hist[(k - c0) * FFA_CALIB_BINS + (lane & 1) * 256 + (lane >> 1) * 255], c);
          }
          cnt[k] = 0u;
        }
      }
    };
    long long ti = blockIdx.x;
    if (ti < ntiles) gload(ti);
    for (; ti < ntiles; ti += gridDim.x) {
#pragma unroll
      for (int k = 0; k < MAXP; ++k)
        if (k < np) *reinterpret_cast<uint4*>(tile + loff[k]) = pre[k];
      __syncthreads();  // also orders the zeroing of hist before its first use
      if (ti + gridDim.x < ntiles) gload(ti + gridDim.x);
      // a lane past the end reads the zeros its tile was filled with and counts nowhere
      const long long i = ti * FFA_CALIB_THREADS + tid;
      const int t = i < npix ? (int)tgt[i] : 255;
      const bool valid = i < npix && t < K;  // targets >= K contribute to nothing
      const unsigned char* mine = tile + tid * slots * 16;
      float z[FFA_CE_MAXK];
#pragma unroll
      for (int v = 0; v < MAXP; ++v) {
        if (v < np) {
          const uint4 u = *reinterpret_cast<const uint4*>(mine + v * 16);
          if constexpr (sizeof(T) == 2) {
            z[v * 8 + 0] = __uint_as_float(u.x << 16);
            z[v * 8 + 1] = __uint_as_float(u.x & 0xffff0000u);
            z[v * 8 + 2] = __uint_as_float(u.y << 16);
            z[v * 8 + 3] = __uint_as_float(u.y & 0xffff0000u);
            z[v * 8 + 4] = __uint_as_float(u.z << 16);
            z[v * 8 + 5] = __uint_as_float(u.z & 0xffff0000u);
            z[v * 8 + 6] = __uint_as_float(u.w << 16);
            z[v * 8 + 7] = __uint_as_float(u.w & 0xffff0000u);
          } else {
            z[v * 4 + 0] = __uint_as_float(u.x);
            z[v * 4 + 1] = __uint_as_float(u.y);
            z[v * 4 + 2] = __uint_as_float(u.z);
            z[v * 4 + 3] = __uint_as_float(u.w);
          }
        }
      }
      // the score bytes: class_prob_crop_kernel's arithmetic, operation for operation
      float m = -INFINITY;
#pragma unroll
      for (int k = 0; k < KR; ++k)
        if (k < K) m = fmaxf(m, z[k]);
      float se = 0.f;
#pragma unroll
      for (int k = 0; k < KR; ++k)
        if (k < K) {
          z[k] = expf(z[k] - m);
          se += z[k];
        }
#pragma unroll
      for (int k = 0; k < KR; ++k) {
        if (k >= c0 && k < c1) {  // wave-uniform
          const int q = (int)(uint8_t)rintf(z[k] / se * 255.f);
          const int side = t == k ? 1 : 0;
          unsigned int* h = hist + (k - c0) * FFA_CALIB_BINS;
          if (valid) {
            if (q == 0 || q == 255) cnt[k] += 1u << (8 * (side + (q == 255 ? 2 : 0)));
            else atomicAdd(&h[side * 256 + q], 1u);
          }
        }
      }
      if (++since == 255) {
        drain();
        since = 0;
      }
      __syncthreads();  // the tile buffer is free for the next fill
    }
    drain();
    __syncthreads();
    for (int i = tid; i < bins; i += FFA_CALIB_THREADS)
      if (hist[i]) atomicAdd(&out[(size_t)c0 * FFA_CALIB_BINS + i], (unsigned long long)hist[i]);
    __syncthreads();  // the bins are free for the next chunk
  }
}

template <typename T>
static void calib_hist_launch(int nb, size_t lds, hipStream_t stream, const void* logits, const uint8_t* targets,
                              long long* hist, long long npix, int K, int Cp, int KC) {
#define FFA_CALIB_HIST(KR_) \
  hipLaunchKernelGGL((calib_hist_kernel<T, KR_>), dim3(nb), dim3(FFA_CALIB_THREADS), lds, stream, (const T*)logits, \
                     targets, reinterpret_cast<unsigned long long*>(hist), npix, K, Cp, KC)
  switch ((K + 7) / 8) {
    case 1: FFA_CALIB_HIST(8); break;
    case 2: FFA_CALIB_HIST(16); break;
    case 3: FFA_CALIB_HIST(24); break;
    default: FFA_CALIB_HIST(32); break;
  }
#undef FFA_CALIB_HIST
}

extern "C" int ffa_calib_hist(int dtype, const void* logits, const uint8_t* targets, long long npix, int K, int Cp,
                              long long* hist, hipStream_t stream) {
  FFA_REQUIRE(dtype == FFA_BF16 || dtype == FFA_F32, "calib_hist: unknown dtype %d", dtype);
  FFA_REQUIRE(K >= 1 && K <= FFA_CE_MAXK && Cp % 8 == 0 && Cp >= K && Cp <= FFA_CE_MAXK,
              "calib_hist: unsupported class count %d (pitch %d)", K, Cp);
  // a block-local 32-bit bin holds at most the block's own pixels
  FFA_REQUIRE(npix >= 0 && npix <= (1LL << 31), "calib_hist: bad pixel count %lld", npix);
  if (npix == 0) return 0;
  FFA_REQUIRE(logits && targets && hist, "calib_hist: null pointer");
  FFA_REQUIRE((reinterpret_cast<uintptr_t>(logits) & 15) == 0, "calib_hist: the logits must be 16-byte aligned");
  const int np = Cp / (dtype == FFA_BF16 ? 8 : 4);
  const int tile_bytes = FFA_CALIB_THREADS * (np | 1) * 16;
  const int room = (FFA_CALIB_LDS - tile_bytes) / (FFA_CALIB_BINS * 4);  // classes whose bins fit: 14 at the least
  const int passes = (K + room - 1) / room;
  const int KC = (K + passes - 1) / passes;
  const size_t lds = (size_t)tile_bytes + (size_t)KC * FFA_CALIB_BINS * 4;
  long long nb = (npix + FFA_CALIB_THREADS - 1) / FFA_CALIB_THREADS;
  if (nb > FFA_CALIB_BLOCKS) nb = FFA_CALIB_BLOCKS;
  if (dtype == FFA_BF16) calib_hist_launch<ffa_bf16>((int)nb, lds, stream, logits, targets, hist, npix, K, Cp, KC);
  else calib_hist_launch<float>((int)nb, lds, stream, logits, targets, hist, npix, K, Cp, KC);
  return ffa_check_launch("calib_hist");
}

// ------------------------------------------------------------------------------------------------
// thresholded labels.  One thread per pixel of the crop window, one pass over its logits, like the prediction kernels
// of resample_loss.hip; the thresholds are read once per block into LDS.

static inline int calib_ew_grid(long long items) {
  long long g = (items + FFA_CALIB_THREADS - 1) / FFA_CALIB_THREADS;
  return (int)(g > 256 * 8 ? 256 * 8 : g < 1 ? 1 : g);
}

template <typename T, bool CONF>
__global__ void __launch_bounds__(FFA_CALIB_THREADS)
label_thresholded_crop_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ thr, int fallback,
                              uint8_t* __restrict__ out, int B, int H, int W, int K, int Cp, int y0, int x0, int h,
                              int w) {
  __shared__ int sthr[FFA_CE_MAXK];
  if (threadIdx.x < FFA_CE_MAXK) sthr[threadIdx.x] = threadIdx.x < K ? (int)thr[threadIdx.x] : 256;
  __syncthreads();
  const long long total = (long long)B * h * w;
  const long long plane = (long long)h * w;
  const int nv = Cp / 8;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % w);
    long long p = i / w;
    const int y = (int)(p % h);
    const long long b = p / h;
    const T* src = logits + ((b * H + y0 + y) * W + x0 + x) * Cp;
    float z[FFA_CE_MAXK], e[FFA_CE_MAXK];
#pragma unroll
    for (int v = 0; v < FFA_CE_MAXK / 8; ++v) {
      if (v < nv) {
        float tmp[8];
        ffa_load8<T>(src + v * 8, tmp);
#pragma unroll
        for (int c = 0; c < 8; ++c) z[v * 8 + c] = tmp[c];
      }
    }
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < FFA_CE_MAXK; ++k)
      if (k < K) m = fmaxf(m, z[k]);
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < FFA_CE_MAXK; ++k)
      if (k < K) {
        e[k] = expf(z[k] - m);
        se += e[k];
      }
    float best = -INFINITY;
    int am = fallback, qa = 0;
#pragma unroll
    for (int k = 0; k < FFA_CE_MAXK; ++k)
      if (k < K) {
        const int q = (int)(uint8_t)rintf(e[k] / se * 255.f);
        if (q >= sthr[k] && z[k] > best) {  // strict '>' keeps the lowest passing index on ties
          best = z[k];
          am = k;
          qa = q;
        }
      }
    if (CONF) {
      const long long o = b * 2 * plane + (long long)y * w + x;
      out[o] = (uint8_t)am;
      out[o + plane] = (uint8_t)qa;
    } else {
      out[i] = (uint8_t)am;
    }
  }
}

extern "C" int ffa_predict_thresholded_u8(int dtype, int mode, const void* logits, const uint8_t* thr, int fallback,
                                          uint8_t* out, int B, int H, int W, int K, int Cp, int y0, int x0, int h,
                                          int w, hipStream_t stream) {
  FFA_REQUIRE(logits && thr && out, "predict_thresholded_u8: null pointer");
  FFA_REQUIRE(dtype == FFA_BF16 || dtype == FFA_F32, "predict_thresholded_u8: unknown dtype %d", dtype);
  FFA_REQUIRE(K >= 1 && K <= FFA_CE_MAXK && Cp % 8 == 0 && Cp >= K && Cp <= FFA_CE_MAXK,
              "predict_thresholded_u8: unsupported class count %d (pitch %d)", K, Cp);
  FFA_REQUIRE(B >= 1 && y0 >= 0 && x0 >= 0 && h > 0 && w > 0 && y0 + h <= H && x0 + w <= W,
              "predict_thresholded_u8: crop outside the tile");
  FFA_REQUIRE(mode == 0 || mode == 2,
              "predict_thresholded_u8: mode %d (0 label, 2 label + confidence; thresholds do not apply to mode 1)", mode);
  FFA_REQUIRE(fallback >= 0 && fallback <= 255, "predict_thresholded_u8: fallback %d is not a uint8 value", fallback);
  const long long items = (long long)B * h * w;
#define FFA_THR(TT, CONF_) \
  hipLaunchKernelGGL((label_thresholded_crop_kernel<TT, CONF_>), dim3(calib_ew_grid(items)), dim3(FFA_CALIB_THREADS), 0, \
                     stream, (const TT*)logits, thr, fallback, out, B, H, W, K, Cp, y0, x0, h, w)
  if (mode == 0) {
    if (dtype == FFA_BF16) FFA_THR(ffa_bf16, false); else FFA_THR(float, false);
  } else {
    if (dtype == FFA_BF16) FFA_THR(ffa_bf16, true); else FFA_THR(float, true);
  }
#undef FFA_THR
  return ffa_check_launch("predict_thresholded_u8");
}

template <bool CONF>
__global__ void __launch_bounds__(FFA_CALIB_THREADS)
tta_label_thresholded_kernel(const float* __restrict__ acc, const uint8_t* __restrict__ thr, int fallback,
                             uint8_t* __restrict__ out, long long total, long long plane, int K, int Cp, float views) {
  __shared__ int sthr[FFA_CE_MAXK];
  if (threadIdx.x < FFA_CE_MAXK) sthr[threadIdx.x] = threadIdx.x < K ? (int)thr[threadIdx.x] : 256;
  __syncthreads();
  const int nv = Cp / 4;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long b = i / plane, pix = i - b * plane;
    const float4* src = reinterpret_cast<const float4*>(acc + i * Cp);
    float p[FFA_CE_MAXK];
#pragma unroll
    for (int v = 0; v < FFA_CE_MAXK / 4; ++v) {
      if (v < nv) {
        const float4 t = src[v];
        p[v * 4] = t.x / views;
        p[v * 4 + 1] = t.y / views;
        p[v * 4 + 2] = t.z / views;
        p[v * 4 + 3] = t.w / views;
      }
    }
    float best = -INFINITY;
    int am = fallback, qa = 0;
#pragma unroll
    for (int k = 0; k < FFA_CE_MAXK; ++k)
      if (k < K) {
        const int q = (int)(uint8_t)rintf(p[k] * 255.f);
        if (q >= sthr[k] && p[k] > best) {  // strict '>' keeps the lowest passing index on ties
          best = p[k];
          am = k;
          qa = q;
        }
      }
    if (CONF) {
      uint8_t* o = out + b * 2 * plane + pix;
      o[0] = (uint8_t)am;
      o[plane] = (uint8_t)qa;
    } else {
      out[i] = (uint8_t)am;
    }
  }
}

extern "C" int ffa_tta_predict_thresholded_u8(int mode, const float* acc, const uint8_t* thr, int fallback,
                                              uint8_t* out, int B, int K, int Cp, int h, int w, int views,
                                              hipStream_t stream) {
  FFA_REQUIRE(acc && thr && out && B >= 1, "tta_predict_thresholded_u8: bad arguments");
  FFA_REQUIRE(K >= 1 && K <= FFA_CE_MAXK && Cp % 8 == 0 && Cp >= K && Cp <= FFA_CE_MAXK,
              "tta_predict_thresholded_u8: unsupported class count %d (pitch %d)", K, Cp);
  FFA_REQUIRE(h > 0 && w > 0, "tta_predict_thresholded_u8: empty window %d x %d", h, w);
  FFA_REQUIRE(views >= 1, "tta_predict_thresholded_u8: %d views", views);
  FFA_REQUIRE(mode == 0 || mode == 2,
              "tta_predict_thresholded_u8: mode %d (0 label, 2 label + confidence; thresholds do not apply to mode 1)",
              mode);
  FFA_REQUIRE(fallback >= 0 && fallback <= 255, "tta_predict_thresholded_u8: fallback %d is not a uint8 value",
              fallback);
  const long long plane = (long long)h * w, total = B * plane;
#define FFA_TTA_THR(CONF_) \
  hipLaunchKernelGGL(tta_label_thresholded_kernel<CONF_>, dim3(calib_ew_grid(total)), dim3(FFA_CALIB_THREADS), 0, \
                     stream, acc, thr, fallback, out, total, plane, K, Cp, (float)views)
  if (mode == 0) FFA_TTA_THR(false);
  else FFA_TTA_THR(true);
#undef FFA_TTA_THR
  return ffa_check_launch("tta_predict_thresholded_u8");
}
