// Test-time augmentation for the zonal tile loop: the inverse path of csrc/augment.hip.  A tile is predicted under
// several flips / rotations ("views", flairhip/augment.py codes); each view's logits come back in the VIEW's frame.
// ffa_tta_accumulate takes one view's softmax probabilities back to the tile's frame and adds them into an f32
// accumulator over the margin-crop window; ffa_tta_predict_u8 / ffa_tta_probabilities turn the accumulator into the
// three uint8 outputs of ffa_predict_u8 / the mean probabilities.  Probabilities are averaged, not logits: the
// class_prob and confidence outputs are probabilities and stay on their scale.
//
// Frames.  view = apply_code(tile, code), so tile[Y, X] = view[si, sj] with (si, sj) the gather of
// inverse_code(code).  In the (swap, fi, fj) form of d4_decode (augment.hip) a code without swap is its own inverse and
// one with swap has the inverse (swap, fj, fi): the host decodes and inverts, the kernel only sees the three flags.
//
// Accumulator: f32, pixel-major over the crop window, [B][h][w][Cp] -- the logits' own pitch, pad channels hold 0 -- so
// a pixel is one record of Cp * 4 bytes and a window row one contiguous run.
//
// Both sides move whole lines: a block owns one 16 x 16 destination tile of one sample; its pre-image in the view is
// again an axis-aligned rectangle, read row by row with 16-byte loads (one thread per source pixel, which takes the
// softmax there in the arithmetic of class_prob_crop_kernel).  The probabilities go through LDS, and the destination
// records are then read-modify-written in memory order, 16 bytes per lane, consecutive lanes on consecutive addresses:
// for odd k the transposition happens in LDS (row pitch (16 + 1) pixels: the 16-lane groups of a 16-byte LDS read fall
// on distinct banks for every pitch in use), never in global memory.  One thread owns an accumulator element and views
// are accumulated in call order: no atomics, deterministic.
#include "ffa_common.h"

#define FFA_TTA_THREADS 256
#define FFA_TTA_TS 16                      // destination tile: 16 x 16 pixels, one thread per source pixel
#define FFA_TTA_PITCH (FFA_TTA_TS + 1)     // LDS row pitch in pixels

struct TtaMap {
  int swap, fi, fj;  // of the INVERSE transform: source row follows the destination column; mirrored source row / column
};

// forward code -> the (swap, fi, fj) of its inverse (d4_decode's closed form, then the inversion above)
static TtaMap tta_inverse_map(int code) {
  const int k = (code >> 2) & 3;
  const int swap = k & 1;
  const int fi = (k >> 1) ^ ((code >> 1) & 1);
  const int fj = ((k == 1 || k == 2) ? 1 : 0) ^ (code & 1);
  TtaMap m;
  m.swap = swap;
  m.fi = swap ? fj : fi;
  m.fj = swap ? fi : fj;
  return m;
}

// grid: B * ceil(h / 16) * ceil(w / 16) blocks; dynamic LDS: 16 * 17 * Cp floats
template <typename T>
__global__ void __launch_bounds__(FFA_TTA_THREADS)
tta_accumulate_kernel(const T* __restrict__ logits, float* __restrict__ acc, int n, int K, int Cp, int y0, int x0,
                      int h, int w, TtaMap m, int first) {
  extern __shared__ float4 tta_tile[];  // [FFA_TTA_TS][FFA_TTA_PITCH][Cp / 4]
  const int ntx = (w + FFA_TTA_TS - 1) / FFA_TTA_TS, nty = (h + FFA_TTA_TS - 1) / FFA_TTA_TS;
  const int tile = blockIdx.x % (ntx * nty);
  const long long b = blockIdx.x / (ntx * nty);
  const int i0 = (tile / ntx) * FFA_TTA_TS, j0 = (tile % ntx) * FFA_TTA_TS;  // destination tile, in the crop window
  const int th = min(FFA_TTA_TS, h - i0), tw = min(FFA_TTA_TS, w - j0);
  // its pre-image in the view: rows follow the destination rows (columns when swapped), mirrored about the plane
  const int a0 = m.swap ? x0 + j0 : y0 + i0, al = m.swap ? tw : th;
  const int b0 = m.swap ? y0 + i0 : x0 + j0, bl = m.swap ? th : tw;
  const int si0 = m.fi ? n - a0 - al : a0, sj0 = m.fj ? n - b0 - bl : b0;
  const int pieces = Cp / 4;

  // ---- one thread per source pixel: softmax there, probabilities -> LDS ----
  {
    const int r = threadIdx.x / FFA_TTA_TS, c = threadIdx.x % FFA_TTA_TS;
    if (r < al && c < bl) {
      const T* src = logits + ((b * n + si0 + r) * n + sj0 + c) * Cp;
      const int nv = Cp / 8;
      float z[FFA_CE_MAXK];
#pragma unroll
      for (int v = 0; v < FFA_CE_MAXK / 8; ++v) {
        if (v < nv) {
          float tmp[8];
          ffa_load8<T>(src + v * 8, tmp);
#pragma unroll
          for (int e = 0; e < 8; ++e) z[v * 8 + e] = tmp[e];
        }
      }
      float mx = -INFINITY;
#pragma unroll
      for (int k = 0; k < FFA_CE_MAXK; ++k)
        if (k < K) mx = fmaxf(mx, z[k]);
      float se = 0.f;
#pragma unroll
      for (int k = 0; k < FFA_CE_MAXK; ++k)
        if (k < K) {
          z[k] = expf(z[k] - mx);
          se += z[k];
        }
#pragma unroll
      for (int k = 0; k < FFA_CE_MAXK; ++k) z[k] = k < K ? z[k] / se : 0.f;
      float4* t = tta_tile + (r * FFA_TTA_PITCH + c) * pieces;
#pragma unroll
      for (int v = 0; v < FFA_CE_MAXK / 4; ++v)
        if (v < pieces) t[v] = make_float4(z[v * 4], z[v * 4 + 1], z[v * 4 + 2], z[v * 4 + 3]);
    }
  }
  __syncthreads();

  // ---- destination records in memory order, 16 bytes per lane ----
  float4* dst = reinterpret_cast<float4*>(acc);
  const int row_pieces = tw * pieces;
  for (int e = threadIdx.x; e < th * row_pieces; e += FFA_TTA_THREADS) {
    const int li = e / row_pieces, rest = e - li * row_pieces;
    const int lj = rest / pieces, q = rest - lj * pieces;
    const int a = m.swap ? lj : li, bb = m.swap ? li : lj;
    const int r = m.fi ? al - 1 - a : a, c = m.fj ? bl - 1 - bb : bb;
    const float4 p = tta_tile[(r * FFA_TTA_PITCH + c) * pieces + q];
    float4* o = dst + ((b * h + i0 + li) * w + j0 + lj) * pieces + q;
    if (first) {
      *o = p;
    } else {
      float4 s = *o;
      s.x += p.x;
      s.y += p.y;
      s.z += p.z;
      s.w += p.w;
      *o = s;
    }
  }
}

extern "C" int ffa_tta_accumulate(int dtype, const void* logits, float* acc, int B, int H, int W, int K, int Cp, int y0,
                                  int x0, int h, int w, int code, int first, hipStream_t stream) {
  FFA_REQUIRE(logits && acc && B >= 1, "tta_accumulate: bad arguments");
  FFA_REQUIRE(dtype == FFA_BF16 || dtype == FFA_F32, "tta_accumulate: unknown dtype %d", dtype);
  FFA_REQUIRE(K >= 1 && K <= FFA_CE_MAXK && Cp % 8 == 0 && Cp >= K && Cp <= FFA_CE_MAXK,
              "tta_accumulate: unsupported class count %d (pitch %d)", K, Cp);
  if (H != W || H < 1) {
    ffa_set_error("tta_accumulate: rotations need square tiles, got %d x %d", H, W);
    return FFA_ERR_UNSUPPORTED;
  }
  FFA_REQUIRE(y0 >= 0 && x0 >= 0 && h > 0 && w > 0 && y0 + h <= H && x0 + w <= W,
              "tta_accumulate: crop outside the tile");
  FFA_REQUIRE(code >= 0 && code <= 15, "tta_accumulate: code %d outside 0..15", code);
  const long long blocks = (long long)B * ((h + FFA_TTA_TS - 1) / FFA_TTA_TS) * ((w + FFA_TTA_TS - 1) / FFA_TTA_TS);
  FFA_REQUIRE(blocks <= 0x7fffffffLL, "tta_accumulate: too many tiles");
  const TtaMap m = tta_inverse_map(code);
  const size_t lds = (size_t)FFA_TTA_TS * FFA_TTA_PITCH * Cp * sizeof(float);
  if (dtype == FFA_BF16)
    hipLaunchKernelGGL(tta_accumulate_kernel<ffa_bf16>, dim3((unsigned)blocks), dim3(FFA_TTA_THREADS), lds, stream,
                       (const ffa_bf16*)logits, acc, H, K, Cp, y0, x0, h, w, m, first != 0);
  else
    hipLaunchKernelGGL(tta_accumulate_kernel<float>, dim3((unsigned)blocks), dim3(FFA_TTA_THREADS), lds, stream,
                       (const float*)logits, acc, H, K, Cp, y0, x0, h, w, m, first != 0);
  return ffa_check_launch("tta_accumulate");
}

// ------------------------------------------------------------------------------------------------
// accumulator -> outputs.  One thread per pixel reads its record and writes one element per output plane (a wave
// writes 64 consecutive elements of each plane), like the prediction kernels of resample_loss.hip.
// MODE 0 / 1 / 2: ffa_predict_u8's outputs; MODE 3: the mean probabilities as f32 [B][K][h][w].

template <int MODE>
__global__ void tta_finish_kernel(const float* __restrict__ acc, void* __restrict__ out, long long total,
                                  long long plane, int K, int Cp, float views) {
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
    if (MODE == 1) {
      uint8_t* o = (uint8_t*)out + b * K * plane + pix;
#pragma unroll
      for (int k = 0; k < FFA_CE_MAXK; ++k)
        if (k < K) o[k * plane] = (uint8_t)rintf(p[k] * 255.f);
    } else if (MODE == 3) {
      float* o = (float*)out + b * K * plane + pix;
#pragma unroll
      for (int k = 0; k < FFA_CE_MAXK; ++k)
        if (k < K) o[k * plane] = p[k];
    } else {
      float top = -INFINITY;
      int am = 0;
#pragma unroll
      for (int k = 0; k < FFA_CE_MAXK; ++k)
        if (k < K && p[k] > top) {  // strict '>' keeps the lowest index on ties
          top = p[k];
          am = k;
        }
      if (MODE == 0) {
        ((uint8_t*)out)[i] = (uint8_t)am;
      } else {
        uint8_t* o = (uint8_t*)out + b * 2 * plane + pix;
        o[0] = (uint8_t)am;
        o[plane] = (uint8_t)rintf(top * 255.f);  // rintf(p * 255) is monotone in p: the largest mode-1 band
      }
    }
  }
}

static int tta_finish_grid(long long items) {
  long long g = (items + FFA_TTA_THREADS - 1) / FFA_TTA_THREADS;
  return (int)(g > 256 * 8 ? 256 * 8 : g < 1 ? 1 : g);
}

static int tta_finish_check(const char* what, const void* acc, const void* out, int B, int K, int Cp, int h, int w,
                            int views) {
  FFA_REQUIRE(acc && out && B >= 1, "%s: bad arguments", what);
  FFA_REQUIRE(K >= 1 && K <= FFA_CE_MAXK && Cp % 8 == 0 && Cp >= K && Cp <= FFA_CE_MAXK,
              "%s: unsupported class count %d (pitch %d)", what, K, Cp);
  FFA_REQUIRE(h > 0 && w > 0, "%s: empty window %d x %d", what, h, w);
  FFA_REQUIRE(views >= 1, "%s: %d views", what, views);
  return 0;
}

extern "C" int ffa_tta_predict_u8(int mode, const float* acc, uint8_t* out, int B, int K, int Cp, int h, int w,
                                  int views, hipStream_t stream) {
  if (int rc = tta_finish_check("tta_predict_u8", acc, out, B, K, Cp, h, w, views)) return rc;
  FFA_REQUIRE(mode == 0 || mode == 1 || mode == 2, "tta_predict_u8: unknown mode %d", mode);
  const long long plane = (long long)h * w, total = B * plane;
#define FFA_TTA_FINISH(M) \
  hipLaunchKernelGGL(tta_finish_kernel<M>, dim3(tta_finish_grid(total)), dim3(FFA_TTA_THREADS), 0, stream, acc, \
                     (void*)out, total, plane, K, Cp, (float)views)
  if (mode == 0) FFA_TTA_FINISH(0);
  else if (mode == 1) FFA_TTA_FINISH(1);
  else FFA_TTA_FINISH(2);
  return ffa_check_launch("tta_predict_u8");
}

extern "C" int ffa_tta_probabilities(const float* acc, float* out, int B, int K, int Cp, int h, int w, int views,
                                     hipStream_t stream) {
  if (int rc = tta_finish_check("tta_probabilities", acc, out, B, K, Cp, h, w, views)) return rc;
  const long long plane = (long long)h * w, total = B * plane;
  FFA_TTA_FINISH(3);
#undef FFA_TTA_FINISH
  return ffa_check_launch("tta_probabilities");
}
