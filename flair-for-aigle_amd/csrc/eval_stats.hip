// libflairhip: what an evaluation needs from the logits, in one pass (ffa_eval_stats).
//
// Per pixel: the label (first maximum over the K real classes), the unweighted cross-entropy term
// -log softmax[target] and one (target, label) count.  Per call: pred[npix], confmat[K][K] += counts,
// class_count[k] = pixels with target k, class_nll[k] = sum over those pixels of (log sum_j exp z_j - z_k).
// The reference's validation loop pays for the per-class loss with a second forward per task and K host reads per
// batch (flair_hub/tasks/tasks_module.py:280-300); its test stage takes argmax and the confusion matrix on the host
// (flair_hub/writer/prediction_writer.py).
//
// The per-pixel arithmetic is softmax_ce_kernel's (f32: maximum, __expf(z - m), sum in class order, __logf(se), the
// target's term as z_t - m itself, kept from before the exponentials: __logf(__expf(z_t - m)) would be -inf once the
// exponential underflows, 87 below the maximum).
// The thread <-> pixel assignment is that of softmax_ce_tiled_kernel, whose staging
// of the logits through LDS in memory order is reused: a thread that owns a 64-byte pixel otherwise touches 32 cache
// lines per wave instruction.
//
// Reduction order of class_nll (no floating-point atomics anywhere; equal inputs give equal bytes):
//   1. thread `tid` of a block adds the terms of its pixels, in the order of its tiles (blockIdx.x, + gridDim.x, ...),
//      into its own f32 cell acc[target][tid] of an LDS column: consecutive lanes are consecutive banks, no conflicts;
//   2. at block end wave w takes classes w, w + 4, ...: lane l adds cells l, l + 64, l + 128, l + 192 in that order,
//      then the fixed xor-shuffle tree of ffa_wave_sum -> parts_nll[block][k] (f32);
//   3. eval_finalize_kernel, one wave per class: lane l adds the blocks' partials l, l + 64, ... in double, then the
//      same tree in double -> class_nll[k].
// Counts are integers: a block-local histogram in LDS with integer atomics (confusion_kernel's pattern), its rows summed
// per block into parts_cnt[block][k] and over the blocks in eval_finalize_kernel; confmat takes one 64-bit integer atomic
// per non-empty bin per block.  Integer addition is exact and order independent.
#include "ffa_common.h"

#define FFA_EVAL_THREADS 256
#define FFA_EVAL_BLOCKS 1024  // grid cap: a block walks tiles blockIdx.x, + gridDim.x, ...

// KR: the class count rounded up to a multiple of 8 -- sizes the LDS column and the histogram, so that 19 classes in
// bf16 leave room for three blocks per CU
template <typename T, int KR>
__global__ void __launch_bounds__(FFA_EVAL_THREADS)
eval_stats_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ tgt, uint8_t* __restrict__ pred,
                  unsigned long long* __restrict__ confmat, float* __restrict__ parts_nll,
                  unsigned int* __restrict__ parts_cnt, long long npix, int K, int Cp) {
  constexpr int EPP = 16 / (int)sizeof(T);  // elements per 16-byte piece
  constexpr int MAXP = FFA_CE_MAXK / EPP;   // pieces per pixel at the largest pitch: 4 (bf16) / 8 (f32)
  __shared__ __align__(16) unsigned char tile[FFA_EVAL_THREADS * (MAXP + 1) * 16];
  __shared__ float acc[KR * FFA_EVAL_THREADS];
  __shared__ unsigned int hist[KR * KR];
  const int tid = threadIdx.x;
  const bool stats = parts_nll != nullptr;
  const bool counts = stats || confmat != nullptr;
  if (stats) {
#pragma unroll
    for (int k = 0; k < KR; ++k) acc[k * FFA_EVAL_THREADS + tid] = 0.f;
  }
  for (int i = tid; i < KR * KR; i += FFA_EVAL_THREADS) hist[i] = 0u;
  const int np = Cp / EPP;   // pieces per pixel
  const int slots = np | 1;  // LDS pitch of a pixel in 16-byte slots: odd
  const long long ntiles = (npix + FFA_EVAL_THREADS - 1) / FFA_EVAL_THREADS;
  int loff[MAXP];  // LDS byte offset of piece tid + 256 k of a tile
#pragma unroll
  for (int k = 0; k < MAXP; ++k) {
    const int idx = tid + FFA_EVAL_THREADS * k;
    loff[k] = ((idx / np) * slots + idx % np) * 16;
  }
  uint4 pre[MAXP];
  auto gload = [&](long long ti) {
    const long long base = ti * FFA_EVAL_THREADS;
    const long long left = npix - base;
    const int npc = (int)(left < FFA_EVAL_THREADS ? left : FFA_EVAL_THREADS) * np;
    const uint4* src = reinterpret_cast<const uint4*>(logits + base * Cp);
#pragma unroll
    for (int k = 0; k < MAXP; ++k) {
      const int idx = tid + FFA_EVAL_THREADS * k;
      if (k < np) pre[k] = idx < npc ? src[idx] : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  long long ti = blockIdx.x;
  if (ti < ntiles) gload(ti);
  for (; ti < ntiles; ti += gridDim.x) {
#pragma unroll
    for (int k = 0; k < MAXP; ++k)
      if (k < np) *reinterpret_cast<uint4*>(tile + loff[k]) = pre[k];
    __syncthreads();  // also orders the zeroing of acc / hist before their first use
    if (ti + gridDim.x < ntiles) gload(ti + gridDim.x);
    const long long i = ti * FFA_EVAL_THREADS + tid;
    if (i < npix) {
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
      float m = -INFINITY;
      int am = 0;
#pragma unroll
      for (int k = 0; k < KR; ++k) {
        if (k < K && z[k] > m) {  // strict '>' keeps the lowest index on ties (torch.argmax)
          m = z[k];
          am = k;
        }
      }
      if (pred) pred[i] = (uint8_t)am;
      const int t = tgt[i];
      if (counts && t < K) {  // targets >= K contribute to nothing
        atomicAdd(&hist[t * K + am], 1u);
        if (stats) {
          float se = 0.f, dt = 0.f;
#pragma unroll
          for (int k = 0; k < KR; ++k) {
            if (k < K) {
              const float d = z[k] - m;
              if (k == t) dt = d;
              se += __expf(d);
            }
          }
          // -log softmax[t] = log(se) - (z_t - m), as in softmax_ce_kernel.  Taken as __logf(__expf(z_t - m)) the second
          // term is -inf once z_t lies 87 below the maximum (an untrained model does that): the sum of a class would
          // be inf where the loss of the pixel is a finite 87.  The difference itself is exact to an f32 rounding.
          acc[t * FFA_EVAL_THREADS + tid] += __logf(se) - dt;  // this thread's own cell
        }
      }
    }
    __syncthreads();  // the tile buffer is free for the next fill
  }
  __syncthreads();  // a block without tiles (npix == 0) still zeroed acc / hist above
  if (stats) {
    const int lane = tid & 63;
    for (int k = tid >> 6; k < KR; k += FFA_EVAL_THREADS / 64) {
      const float* col = acc + k * FFA_EVAL_THREADS;
      float s = ((col[lane] + col[lane + 64]) + col[lane + 128]) + col[lane + 192];
      s = ffa_wave_sum(s);
      if (lane == 0) parts_nll[(size_t)blockIdx.x * FFA_CE_MAXK + k] = s;
    }
    if (tid < KR) {
      unsigned int c = 0u;
      if (tid < K)
        for (int p = 0; p < K; ++p) c += hist[tid * K + p];
      parts_cnt[(size_t)blockIdx.x * FFA_CE_MAXK + tid] = c;
    }
  }
  if (confmat) {
    const int bins = K * K;
    for (int i = tid; i < bins; i += FFA_EVAL_THREADS)
      if (hist[i]) atomicAdd(&confmat[i], (unsigned long long)hist[i]);
  }
}

// one wave per class: lane l adds block partials l, l + 64, ... (double / int64), then a fixed xor-shuffle tree
__global__ void __launch_bounds__(64)
eval_finalize_kernel(const float* __restrict__ parts_nll, const unsigned int* __restrict__ parts_cnt, int nb,
                     double* __restrict__ class_nll, long long* __restrict__ class_count) {
  const int k = blockIdx.x;
  double s = 0.0;
  long long c = 0;
  for (int i = threadIdx.x; i < nb; i += 64) {
    s += (double)parts_nll[(size_t)i * FFA_CE_MAXK + k];
    c += (long long)parts_cnt[(size_t)i * FFA_CE_MAXK + k];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    c += __shfl_xor(c, o, 64);
  }
  if (threadIdx.x == 0) {
    class_nll[k] = s;
    class_count[k] = c;
  }
}

extern "C" long long ffa_eval_stats_workspace_bytes(void) {
  // per block and class: one f32 loss partial and one u32 count
  return (long long)FFA_EVAL_BLOCKS * FFA_CE_MAXK * (sizeof(float) + sizeof(unsigned int));
}

template <typename T, int KR>
static void eval_stats_launch(int nb, hipStream_t stream, const void* logits, const uint8_t* targets, uint8_t* pred,
                              long long* confmat, float* parts_nll, unsigned int* parts_cnt, long long npix, int K,
                              int Cp) {
  hipLaunchKernelGGL((eval_stats_kernel<T, KR>), dim3(nb), dim3(FFA_EVAL_THREADS), 0, stream, (const T*)logits, targets,
                     pred, reinterpret_cast<unsigned long long*>(confmat), parts_nll, parts_cnt, npix, K, Cp);
}

template <typename T>
static void eval_stats_dispatch(int nb, hipStream_t stream, const void* logits, const uint8_t* targets, uint8_t* pred,
                                long long* confmat, float* parts_nll, unsigned int* parts_cnt, long long npix, int K,
                                int Cp) {
  switch ((K + 7) / 8) {
    case 1: return eval_stats_launch<T, 8>(nb, stream, logits, targets, pred, confmat, parts_nll, parts_cnt, npix, K, Cp);
    case 2: return eval_stats_launch<T, 16>(nb, stream, logits, targets, pred, confmat, parts_nll, parts_cnt, npix, K, Cp);
    case 3: return eval_stats_launch<T, 24>(nb, stream, logits, targets, pred, confmat, parts_nll, parts_cnt, npix, K, Cp);
    default: return eval_stats_launch<T, 32>(nb, stream, logits, targets, pred, confmat, parts_nll, parts_cnt, npix, K, Cp);
  }
}

// pred, confmat and the pair (class_nll, class_count) may each be null and are then skipped; confmat accumulates,
// class_nll / class_count are overwritten.  The logits must be 16-byte aligned (every tensor of the library is).
extern "C" int ffa_eval_stats(int dtype, const void* logits, const uint8_t* targets, long long npix, int K, int Cp,
                              uint8_t* pred, long long* confmat, double* class_nll, long long* class_count,
                              void* workspace, long long workspace_bytes, hipStream_t stream) {
  FFA_REQUIRE(dtype == FFA_BF16 || dtype == FFA_F32, "eval_stats: unknown dtype %d", dtype);
  FFA_REQUIRE(K >= 1 && K <= FFA_CE_MAXK && Cp % 8 == 0 && Cp >= K && Cp <= FFA_CE_MAXK,
              "eval_stats: unsupported class count %d (pitch %d)", K, Cp);
  FFA_REQUIRE(npix >= 0 && npix <= (1LL << 40), "eval_stats: bad pixel count %lld", npix);
  FFA_REQUIRE((logits && targets) || npix == 0, "eval_stats: null pointer");
  FFA_REQUIRE((reinterpret_cast<uintptr_t>(logits) & 15) == 0, "eval_stats: the logits must be 16-byte aligned");
  FFA_REQUIRE((class_nll != nullptr) == (class_count != nullptr), "eval_stats: class_nll and class_count go together");
  float* parts_nll = nullptr;
  unsigned int* parts_cnt = nullptr;
  if (class_nll) {
    FFA_REQUIRE(workspace, "eval_stats: null workspace");
    if (workspace_bytes < ffa_eval_stats_workspace_bytes()) {
      ffa_set_error("eval_stats: workspace too small");
      return FFA_ERR_WORKSPACE;
    }
    parts_nll = static_cast<float*>(workspace);
    parts_cnt = reinterpret_cast<unsigned int*>(parts_nll + (size_t)FFA_EVAL_BLOCKS * FFA_CE_MAXK);
  }
  if (!pred && !confmat && !class_nll) return 0;
  long long nb = (npix + FFA_EVAL_THREADS - 1) / FFA_EVAL_THREADS;
  if (nb > FFA_EVAL_BLOCKS) nb = FFA_EVAL_BLOCKS;
  if (nb < 1) nb = 1;  // npix == 0: one block that finds no tile and leaves zero partials
  if (dtype == FFA_BF16)
    eval_stats_dispatch<ffa_bf16>((int)nb, stream, logits, targets, pred, confmat, parts_nll, parts_cnt, npix, K, Cp);
  else
    eval_stats_dispatch<float>((int)nb, stream, logits, targets, pred, confmat, parts_nll, parts_cnt, npix, K, Cp);
  if (class_nll)
    hipLaunchKernelGGL(eval_finalize_kernel, dim3(K), dim3(64), 0, stream, parts_nll, parts_cnt, (int)nb, class_nll,
                       class_count);
  return ffa_check_launch("eval_stats");
}
