// Implicit-GEMM convolution on MFMA for gfx950, NHWC, bf16 or f32 operands, f32 accumulate.
//
// Replaces the cuDNN/ATen conv2d reached through segmentation_models_pytorch from
// flair_hub/models/monotemp_model.py:68-92 (encoder/decoder conv stack called at
// flair_hub/models/flair_model.py:376 and :417-419).  The same kernel serves
//   * forward conv (3x3 s1/s2, 1x1 s1/s2, 7x7 s2) with fused bias / residual add / ReLU epilogue
//   * dgrad: a stride-1 conv over dy with flipped+transposed packed weights; for stride-2
//     layers dy is read through a virtual zero-insertion (dil = 2), never materialised.
//
// GEMM orientation: D[co][pixel] = W[co][k] * X[k][pixel], k = (tap, channel).  Weights are the
// MFMA A operand (rows), pixels the B operand (columns), so every lane ends up holding runs of
// consecutive output channels of ONE pixel -> 16-byte NHWC stores without an LDS transpose.
//
// Per block: BCO output channels x (TH x TW) output pixels of one image.  Per chunk (one 32-byte
// k-step of input channels, RG kernel rows): the input halo tile and the weight slab are staged
// global -> registers -> LDS (zero fill for padding / zero-insertion happens in registers), the
// next chunk's global loads are issued before the MFMAs of the current one.
// LDS images:  halo  [IH*IW pixels][32 B + 16 B pad]  (pitch 48 B: conflict-free ds_read_b128
//                     for 16 consecutive pixels, 3 is coprime with the 16 slots of a bank row)
//              weight [BCO rows][TAPS*32 B + 16 B pad] (odd number of 16-B slots per row)
#include "ffa_gfx950.h"
#include "conv_call.h"

#include <stdlib.h>

#ifndef FFA_CONV_READS_FIRST
#define FFA_CONV_READS_FIRST 0
#endif

// Developer instrumentation (never built by flairhip/build.py): -DFFA_CONV_TRACE=1 makes wave 0 of the first 64
// blocks log s_memtime at every phase boundary into a device buffer read back with ffa_conv_trace_read.
#ifndef FFA_CONV_TRACE
#define FFA_CONV_TRACE 0
#endif
#if FFA_CONV_TRACE
#ifndef FFA_CONV_TRACE_FIRST
#define FFA_CONV_TRACE_FIRST 0
#endif
__device__ long long ffa_conv_trace_buf[64 * 256];
#define FFA_TRACE(slot_)                                                                    \
  if (trace_on) {                                                                           \
    if (trace_n < 256) ffa_conv_trace_buf[(blockIdx.x - FFA_CONV_TRACE_FIRST) * 256 + trace_n] = (long long)(slot_) << 56 | (__builtin_readcyclecounter() & 0xFFFFFFFFFFFFFFLL); \
    ++trace_n;                                                                              \
  }
#else
#define FFA_TRACE(slot_)
#endif

struct ConvArgs {
  const void* in;
  const void* w;      // conv_igemm layout of conv_pack.hip: [cb][cc][rg][row < BCO][tap < RG*KW][32 B]
  void* out;
  const float* bias;  // [>= co block coverage] or null
  float* stats;       // [npt][2][Co] per-tile channel sums / sums of squares of the stored output, or null
  const void* in2;    // UP kernels: the skip tensor [B][Hi][Wi][C2]; `in` is then the low-res map [B][Hi/2][Wi/2][C1]
  int c1_bytes;       // UP kernels: bytes of one pixel of `in` (C1 * sizeof(T)); the virtual input has Ci = C1 + C2
  // BatchNorm-backward partials (bnx != null; needs stats): the tensor written is the gradient dy of
  // y = relu(x * bn_sc + bn_sh); stats then receives per tile (sum g, sum g*x) with g = dy masked by y > 0
  const void* bnx;    // the pre-normalisation tensor x, same shape / pitch as out
  const float* bn_sc;
  const float* bn_sh;
  void* out2;         // split epilogue (c1_out > 0): output channels >= c1_out go here, pixel pitch Co - c1_out
  int c1_out;         // split epilogue: output channels < c1_out are 2x2-sum-pooled into `out` [B][Ho/2][Wo/2][c1_out]
  const void* res;    // same layout as out, or null
  int B, Hi, Wi, Ci;  // stored input dims (Ci = channel pitch)
  int Ho, Wo, Co;     // Co = stored output channel pitch
  int pad, dil, relu;
  int nchunks;  // Ci * sizeof(T) / 32
  int tiles_x, tiles_y, npt, ncb;
};

// HK = 32-byte k-steps of channels staged per halo fill.  With HK = 4 every halo pixel is fetched as one whole
// 128-byte line (64 bf16 channels) and then multiplied over four weight sub-chunks; with HK = 1 each line is
// re-requested from L2 four times, 32 bytes at a time -- measured L2-bound on the 128..256-channel layers.
template <int KH, int KW, int STRIDE, int RG, int BCO, int WCO, int WPX, int TH, int TW, int HK>
struct ConvGeom {
  static constexpr int NTHR = 64 * WCO * WPX;
  static constexpr int NPX = TH * TW;
  static constexpr int WAVE_CO = BCO / WCO;
  static constexpr int MT = WAVE_CO / 32;
  static constexpr int WAVE_PX = NPX / WPX;
  static constexpr int NT = WAVE_PX / 32;
  static constexpr bool ONE = (KH == 1 && KW == 1);
  static constexpr int LS = ONE ? 1 : STRIDE;     // LDS pixel step between neighbouring outputs
  static constexpr int GSTEP = ONE ? STRIDE : 1;  // global pixel step between neighbouring halo pixels
  static constexpr int NRG = KH / RG;
  static constexpr int IH = (TH - 1) * LS + RG;
  static constexpr int IW = (TW - 1) * LS + KW;
  static constexpr int PP = HK * 32 + 16;  // 3 / 5 / 9 slots of 16 B: odd -> conflict-free ds_read_b128
  static constexpr int HPP = 2 * HK;       // 16-byte pieces per halo pixel
  static constexpr int TAPS = RG * KW;
  static constexpr int WP = TAPS * 32 + 16;
  static constexpr int HALO_BYTES = IH * IW * PP;
  static constexpr int W_BYTES = BCO * WP;
  static constexpr int LDS_BYTES = HALO_BYTES + W_BYTES;
  static constexpr int W_PIECES = BCO * TAPS * 2;
  static constexpr int H_PIECES = IH * IW * HPP;
  static constexpr int NWP = (W_PIECES + NTHR - 1) / NTHR;
  static constexpr int NHP = (H_PIECES + NTHR - 1) / NTHR;
  static_assert(KH % RG == 0, "row group must divide kernel height");
  static_assert(HK == 1 || RG == KH, "deep halo staging needs all kernel rows in one chunk");
  static_assert(WAVE_CO == 32 || WAVE_CO == 64, "wave co tile");
  static_assert(WAVE_PX % 32 == 0, "wave px tile");
  static_assert((TW & (TW - 1)) == 0, "TW must be a power of two");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

// UP = the input is the VIRTUAL tensor cat(nearest_x2(in), in2) of a U-Net decoder block (smp DecoderBlock:
// F.interpolate(scale_factor=2, mode="nearest") + torch.cat): channel groups below C1 are fetched from the low-res
// map at (y/2, x/2), the rest from the skip tensor, so the concatenated tensor is never written or re-read.
template <typename T, int KH, int KW, int STRIDE, int RG, int BCO, int WCO, int WPX, int TH, int TW, int HK,
          bool UP = false>
__global__ void __launch_bounds__(64 * WCO * WPX, 2) conv_igemm_kernel(ConvArgs a) {
  static_assert(!UP || (HK >= 2 && KH == 3 && STRIDE == 1), "the two-source loader lives in the pipelined 3x3 path");
  using G = ConvGeom<KH, KW, STRIDE, RG, BCO, WCO, WPX, TH, TW, HK>;
  constexpr int EB = ElemTraits<T>::kBytes;
  __shared__ __align__(16) unsigned char smem[G::LDS_BYTES];
  unsigned char* sIn = smem;
  unsigned char* sW = smem + G::HALO_BYTES;

  // block -> (pixel tile, co block); blocks b and b+8 share an XCD (observed round-robin), so the
  // co blocks of one pixel tile are kept on one XCD's L2 (speed only, never correctness)
  const int bid = blockIdx.x;
  const int xcd = bid & 7;
  const int j = bid >> 3;
  const int pt = (j / a.ncb) * 8 + xcd;
  const int cb = j % a.ncb;
  if (pt >= a.npt) return;
  const int tx = pt % a.tiles_x;
  const int t2 = pt / a.tiles_x;
  const int ty = t2 % a.tiles_y;
  const int b = t2 / a.tiles_y;
  const int oy0 = ty * TH, ox0 = tx * TW;
  const int iy_base = oy0 * STRIDE - a.pad;
  const int ix_base = ox0 * STRIDE - a.pad;

  const int tid = threadIdx.x;
#if FFA_CONV_TRACE
  // FFA_CONV_TRACE_FIRST: first traced block (a later dispatch round shows the steady state)
  const bool trace_on = (threadIdx.x == 0 && (int)blockIdx.x >= FFA_CONV_TRACE_FIRST && (int)blockIdx.x < FFA_CONV_TRACE_FIRST + 64);
  int trace_n = 0;
#endif
  FFA_TRACE(0)
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wco = wave / WPX;
  const int wpx = wave % WPX;
  const int rho = lane & 31;
  const int half = lane >> 5;

  // per-lane LDS fragment offsets
  int aoff[G::MT];
#pragma unroll
  for (int mt = 0; mt < G::MT; ++mt) {
    // LDS rows are stored in fragment order (row mt*32 + rho of a 64-row group holds output channel
    // 16*(rho>>3) + 8*((rho>>2)&1) + 4*mt + (rho&3), the permutation is applied by ffa_pack_conv_weight), so
    // neighbouring lanes read neighbouring rows: 19 slots per row is odd -> conflict-free ds_read_b128
    aoff[mt] = (wco * G::WAVE_CO + mt * 32 + rho) * G::WP + half * 16;
  }
  int boff[G::NT];
#pragma unroll
  for (int nt = 0; nt < G::NT; ++nt) {
    const int n = wpx * G::WAVE_PX + nt * 32 + rho;
    const int py = n / TW, px = n % TW;
    boff[nt] = ((py * G::LS) * G::IW + px * G::LS) * G::PP + half * 16;
  }

  ffa_f32x16 acc[G::MT][G::NT];
#pragma unroll
  for (int mt = 0; mt < G::MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < G::NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

  const unsigned char* in_b = static_cast<const unsigned char*>(a.in);
  const unsigned char* w_b = static_cast<const unsigned char*>(a.w) +
                             (size_t)cb * a.nchunks * G::NRG * (size_t)(BCO * G::TAPS * 32);
  const int total_chunks = a.nchunks * G::NRG;

  ffa_u32x4 wregA[G::NWP], wregB[G::NWP];  // weight slabs of chunk c+1 / c+2 in flight (prefetch distance 2)
  ffa_u32x4 hreg[G::NHP];

  // halo piece geometry, computed once: byte offset from the input base (32-bit: the host checks the tensor is
  // smaller than 2 GiB), -1 where the piece is padding / zero insertion / past the tile; LDS byte address
  int hoff[G::NHP], hlds[G::NHP];
  int hoff2[UP ? G::NHP : 1];  // UP: offsets into the skip tensor (hoff then addresses the low-res map)
#pragma unroll
  for (int k = 0; k < G::NHP; ++k) {
    const int i = tid + k * G::NTHR;
    const int q = i / G::HPP, hh = i % G::HPP;
    const int hy = q / G::IW, hx = q % G::IW;
    int vy = iy_base + hy * G::GSTEP;
    int vx = ix_base + hx * G::GSTEP;
    bool ok = (i < G::H_PIECES) && vy >= 0 && vx >= 0;
    if (a.dil == 2) {
      ok = ok && (((vy | vx) & 1) == 0);
      vy >>= 1;
      vx >>= 1;
    }
    ok = ok && vy < a.Hi && vx < a.Wi;
    if constexpr (UP) {
      hoff[k] = ok ? (((b * (a.Hi >> 1) + (vy >> 1)) * (a.Wi >> 1) + (vx >> 1)) * a.c1_bytes + hh * 16) : -1;
      hoff2[k] = ok ? (((b * a.Hi + vy) * a.Wi + vx) * (a.Ci * EB - a.c1_bytes) + hh * 16) : -1;
    } else {
      hoff[k] = ok ? (((b * a.Hi + vy) * a.Wi + vx) * a.Ci * EB + hh * 16) : -1;
    }
    hlds[k] = q * G::PP + hh * 16;
  }

#define FFA_LOAD_W(c_, WR)                                                                                   \
  {                                                                                                          \
    const ffa_u32x4* wsrc_ = reinterpret_cast<const ffa_u32x4*>(w_b + (size_t)(c_) * (BCO * G::TAPS * 32)); \
    _Pragma("unroll") for (int k = 0; k < G::NWP; ++k) {                                                     \
      const int i = tid + k * G::NTHR;                                                                       \
      WR[k] = wsrc_[(k + 1 < G::NWP || G::W_PIECES % G::NTHR == 0 || i < G::W_PIECES) ? i : 0];                                \
    }                                                                                                        \
  }
  /* c_ = chunk whose halo is needed: channel bytes (c_/NRG/HK)*HK*32 .., kernel rows (c_ % NRG)*RG ..
     The per-piece byte offset and validity are chunk independent (NRG == 1): they were computed once into
     hoff[] (-1 = zero fill), so a refill costs one scalar add for the base and no vector address math. */
#define FFA_LOAD_H(c_)                                                                                       \
  {                                                                                                          \
    const int cbyte_ = (((c_) / G::NRG) / HK) * (HK * 32);                                                   \
    if constexpr (G::NRG == 1) {                                                                             \
      const unsigned char* base_ = in_b + cbyte_;                                                            \
      _Pragma("unroll") for (int k = 0; k < G::NHP; ++k) {                                                   \
        ffa_u32x4 v = ffa_u32x4{0u, 0u, 0u, 0u};                                                             \
        if (hoff[k] >= 0) v = *reinterpret_cast<const ffa_u32x4*>(base_ + (unsigned)hoff[k]);                \
        hreg[k] = v;                                                                                         \
      }                                                                                                      \
    } else {                                                                                                 \
      const int iy0_ = iy_base + ((c_) % G::NRG) * RG;                                                       \
      _Pragma("unroll") for (int k = 0; k < G::NHP; ++k) {                                                   \
        const int i = tid + k * G::NTHR;                                                                     \
        const int q = i / G::HPP;                                                                            \
        const int hh = i % G::HPP;                                                                           \
        const int hy = q / G::IW, hx = q % G::IW;                                                            \
        int vy = iy0_ + hy * G::GSTEP;                                                                       \
        int vx = ix_base + hx * G::GSTEP;                                                                    \
        bool ok = (i < G::H_PIECES) && vy >= 0 && vx >= 0;                                                   \
        if (a.dil == 2) {                                                                                    \
          ok = ok && (((vy | vx) & 1) == 0);                                                                 \
          vy >>= 1;                                                                                          \
          vx >>= 1;                                                                                          \
        }                                                                                                    \
        ok = ok && vy < a.Hi && vx < a.Wi;                                                                   \
        ffa_u32x4 v = ffa_u32x4{0u, 0u, 0u, 0u};                                                             \
        if (ok) {                                                                                            \
          const size_t off =                                                                                 \
              ((size_t)(b * a.Hi + vy) * a.Wi + vx) * (size_t)(a.Ci * EB) + cbyte_ + hh * 16;                \
          v = *reinterpret_cast<const ffa_u32x4*>(in_b + off);                                               \
        }                                                                                                    \
        hreg[k] = v;                                                                                         \
      }                                                                                                      \
    }                                                                                                        \
  }
#define FFA_STORE_W(WR)                                                                    \
  {                                                                                        \
    _Pragma("unroll") for (int k = 0; k < G::NWP; ++k) {                                   \
      const int i = tid + k * G::NTHR;                                                     \
      if (k + 1 < G::NWP || G::W_PIECES % G::NTHR == 0 || i < G::W_PIECES) {                                 \
        const int row = i / (G::TAPS * 2), col = i % (G::TAPS * 2);                        \
        *reinterpret_cast<ffa_u32x4*>(sW + row * G::WP + col * 16) = WR[k];                \
      }                                                                                    \
    }                                                                                      \
  }
#define FFA_STORE_H()                                                                      \
  {                                                                                        \
    _Pragma("unroll") for (int k = 0; k < G::NHP; ++k) {                                   \
      const int i = tid + k * G::NTHR;                                                     \
      if (k + 1 < G::NHP || G::H_PIECES % G::NTHR == 0 || i < G::H_PIECES)                                   \
        *reinterpret_cast<ffa_u32x4*>(sIn + hlds[k]) = hreg[k];                            \
    }                                                                                      \
  }

  // one chunk of matrix work from the LDS images; `sub` = byte offset of the chunk's k-step inside a halo pixel
  // `issue(tap)` = the global loads this chunk sends on behalf of later chunks, spread over the taps so that the
  // texture path (64 B/clk per CU: a block's 29 KB per chunk is ~450 cycles of it) drains under the matrix work
  // instead of in a burst in front of it; `nv(tap)` = how many VMEM instructions that is (for the pinned order)
  auto compute = [&](int sub, auto issue, auto nv) __attribute__((always_inline)) {
    // fragments are double-buffered in registers: the ds_reads of tap t+1 are issued before the MFMAs of
    // tap t, so their LDS latency hides under the matrix pipe instead of stalling every tap
    ffa_u32x4 af[2][G::MT], bf[2][G::NT];
#pragma unroll
    for (int mt = 0; mt < G::MT; ++mt) af[0][mt] = *reinterpret_cast<const ffa_u32x4*>(sW + aoff[mt]);
#pragma unroll
    for (int nt = 0; nt < G::NT; ++nt) bf[0][nt] = *reinterpret_cast<const ffa_u32x4*>(sIn + boff[nt] + sub);
#pragma unroll
    for (int tap = 0; tap < G::TAPS; ++tap) {
      const int cur = tap & 1, nxt = cur ^ 1;
      __builtin_amdgcn_sched_barrier(0);  // one scheduling region per tap: its MFMAs + the reads of the next tap
      issue(tap);
      if (tap + 1 < G::TAPS) {
        const int r1 = (tap + 1) / KW, s1 = (tap + 1) % KW;
#pragma unroll
        for (int mt = 0; mt < G::MT; ++mt)
          af[nxt][mt] = *reinterpret_cast<const ffa_u32x4*>(sW + aoff[mt] + (tap + 1) * 32);
#pragma unroll
        for (int nt = 0; nt < G::NT; ++nt)
          bf[nxt][nt] = *reinterpret_cast<const ffa_u32x4*>(sIn + boff[nt] + sub + (r1 * G::IW + s1) * G::PP);
      }
#pragma unroll
      for (int mt = 0; mt < G::MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < G::NT; ++nt) Mma<T>::run(af[cur][mt], bf[cur][nt], acc[mt][nt]);
      // pin the interleave (hipcc otherwise sinks the reads back to just before their first use):
      // one MFMA group, one ds_read, ... so every read has a full tap of matrix work to land under
      {
        constexpr int NM = G::MT * G::NT;
        const int NR = (tap + 1 < G::TAPS) ? G::MT + G::NT : 0;
        const int NV = nv(tap);
        constexpr int PER = (sizeof(T) == 2) ? 1 : 4;  // MFMAs per Mma<T>::run
#pragma unroll
        for (int i = 0; i < NM; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, PER, 0);
          if (i < NR) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          if (i < NV) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        }
#pragma unroll
        for (int i = NM; i < G::MT + G::NT; ++i)
          if (i < NR) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#pragma unroll
        for (int i = NM; i < NM + 4; ++i)
          if (i < NV) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  };

  // Halo refills are issued HD chunks before they are stored (deep staging: three chunks of matrix work to land
  // under), weight slabs two chunks ahead (two register sets, loop unrolled by two)
  constexpr int HD = (HK >= 4 && G::NRG == 1) ? 3 : 1;
#define FFA_CHUNK(c_, WCUR, WNXT)                                                                            \
  {                                                                                                          \
    const int cq_ = (c_);                                                                                    \
    if (cq_ + 2 < total_chunks) FFA_LOAD_W(cq_ + 2, WNXT)                                                    \
    if (cq_ + HD < total_chunks && (G::NRG > 1 || ((cq_ + HD) % HK) == 0)) FFA_LOAD_H(cq_ + HD)              \
    FFA_TRACE(2)                                                                                             \
    compute((G::NRG > 1) ? 0 : (cq_ % HK) * 32, no_issue, no_nv);                                            \
    FFA_TRACE(3)                                                                                             \
    __syncthreads();                                                                                         \
    FFA_TRACE(4)                                                                                             \
    if (cq_ + 1 < total_chunks) {                                                                            \
      FFA_STORE_W(WCUR)                                                                                      \
      if (G::NRG > 1 || ((cq_ + 1) % HK) == 0) FFA_STORE_H()                                                 \
      FFA_TRACE(5)                                                                                           \
      __syncthreads();                                                                                       \
      FFA_TRACE(6)                                                                                           \
    }                                                                                                        \
  }

  auto no_issue = [](int) __attribute__((always_inline)) {};
  auto no_nv = [](int) __attribute__((always_inline)) { return 0; };

  FFA_LOAD_W(0, wregA)
  FFA_LOAD_H(0)
  FFA_STORE_W(wregA)
  FFA_STORE_H()
  __syncthreads();
  FFA_TRACE(1)
  if (total_chunks > 1) FFA_LOAD_W(1, wregA)
  if constexpr (HK >= 2 && G::NRG == 1) {
    // Pipelined path (3x3 stride 1, whole groups of HK chunks per halo fill): every global load is issued from
    // inside a tap's scheduling region.  Loads are unconditional -- a chunk index past the end is clamped (the
    // data is never stored), a padding piece reads offset 0 and is zeroed when it is stored -- so the regions hold
    // no branches and the pinned MFMA / ds_read / global_load order survives.
    constexpr int HJ = (HK >= 4) ? 1 : 0;  // chunk of the group during which the next group's halo is requested
    const int last_group = total_chunks - HK;
    for (int c0 = 0; c0 < total_chunks; c0 += HK) {
      const int cn = (c0 + HK <= last_group) ? c0 + HK : last_group;  // next group (clamped)
      const int gbn = (cn / HK) * (HK * 32);  // its first channel byte within a (virtual) input pixel
      const bool nextA = !UP || gbn < a.c1_bytes;
      const unsigned char* hbase = nextA ? in_b + gbn : static_cast<const unsigned char*>(a.in2) + (gbn - a.c1_bytes);
#pragma unroll
      for (int j = 0; j < HK; ++j) {
        const int c = c0 + j;
        const int cw = (c + 2 < total_chunks) ? c + 2 : total_chunks - 1;
        const ffa_u32x4* wsrc = reinterpret_cast<const ffa_u32x4*>(w_b + (size_t)cw * (BCO * G::TAPS * 32));
        auto issue = [&](int tap) __attribute__((always_inline)) {
#pragma unroll
          for (int k = 0; k < G::NWP; ++k) {
            if (k % G::TAPS != tap) continue;
            const int i = tid + k * G::NTHR;
            const ffa_u32x4 v = wsrc[(k + 1 < G::NWP || G::W_PIECES % G::NTHR == 0 || i < G::W_PIECES) ? i : 0];
            if (j & 1) wregA[k] = v;
            else wregB[k] = v;
          }
          if (j == HJ) {
#pragma unroll
            for (int k = 0; k < G::NHP; ++k) {
              if (k % G::TAPS != tap) continue;
              int off = hoff[k];
              if constexpr (UP) off = nextA ? hoff[k] : hoff2[k];
              hreg[k] = *reinterpret_cast<const ffa_u32x4*>(hbase + (unsigned)(off >= 0 ? off : 0));
            }
          }
        };
        auto nv = [&](int tap) __attribute__((always_inline)) {
          int n = 0;
#pragma unroll
          for (int k = 0; k < G::NWP; ++k) n += (k % G::TAPS == tap) ? 1 : 0;
          if (j == HJ) {
#pragma unroll
            for (int k = 0; k < G::NHP; ++k) n += (k % G::TAPS == tap) ? 1 : 0;
          }
          return n;
        };
        FFA_TRACE(2)
        compute(j * 32, issue, nv);
        FFA_TRACE(3)
        __syncthreads();
        FFA_TRACE(4)
        if (c + 1 < total_chunks) {
          if (j & 1) FFA_STORE_W(wregB)
          else FFA_STORE_W(wregA)
          if (j == HK - 1) {
#pragma unroll
            for (int k = 0; k < G::NHP; ++k) {
              const int i = tid + k * G::NTHR;
              if (k + 1 < G::NHP || G::H_PIECES % G::NTHR == 0 || i < G::H_PIECES)
                *reinterpret_cast<ffa_u32x4*>(sIn + hlds[k]) = (hoff[k] >= 0) ? hreg[k] : ffa_u32x4{0u, 0u, 0u, 0u};
            }
          }
          FFA_TRACE(5)
          __syncthreads();
          FFA_TRACE(6)
        }
      }
    }
  } else {
    for (int c = 0; c < total_chunks; c += 2) {
      FFA_CHUNK(c, wregA, wregB)
      if (c + 1 < total_chunks) FFA_CHUNK(c + 1, wregB, wregA)
    }
  }

#undef FFA_CHUNK
#undef FFA_LOAD_W
#undef FFA_LOAD_H
#undef FFA_STORE_W
#undef FFA_STORE_H

  // epilogue: lane (rho, half) owns pixel n = wave px base + nt*32 + rho and, per g, a run of
  // consecutive channels (8 for MT==2, 4 for MT==1)
  T* out = static_cast<T*>(a.out);
  const T* res = static_cast<const T*>(a.res);
  const int co_wave = cb * BCO + wco * G::WAVE_CO;
  int opitch = a.Co, cshift = 0;  // pixel pitch of the tensor written and the channel it starts at
  if (a.c1_out > 0) {
    // Split epilogue = backward of "nearest x2 upsample + concat" fused into the dgrad of a decoder block's first
    // conv: the gradient of the virtual input cat(up(lo), skip) never exists as a tensor.  Channel blocks below
    // c1_out are summed over their 2x2 pixel quads (the adjoint of nearest x2) and written at half resolution,
    // the rest goes to the skip-gradient tensor with its own pitch.
    if (cb * BCO >= a.c1_out) {
      out = static_cast<T*>(a.out2);
      opitch = a.Co - a.c1_out;
      cshift = a.c1_out;
    } else {
      static_assert(G::WAVE_PX == 64, "quad pooling assumes two 32-pixel fragments per wave");
      constexpr int NV = (G::MT == 2) ? 8 : 4;
      const int Hl = a.Ho >> 1, Wl = a.Wo >> 1;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c0 = (G::MT == 2) ? co_wave + 16 * g + 8 * half : co_wave + 8 * g + 4 * half;
        float q[G::NT][NV];
#pragma unroll
        for (int nt = 0; nt < G::NT; ++nt) {
          const int n = wpx * G::WAVE_PX + nt * 32 + rho;
          const bool ok = (oy0 + n / TW) < a.Ho && (ox0 + n % TW) < a.Wo;
#pragma unroll
          for (int i = 0; i < NV; ++i) {
            const float v = (G::MT == 2) ? acc[i >> 2][nt][4 * g + (i & 3)] : acc[0][nt][4 * g + i];
            q[nt][i] = ok ? v : 0.f;
          }
        }
        if (TW == 32) {  // fragment nt = tile row 2*wpx + nt, lane = column: vertical partner in registers
#pragma unroll
          for (int i = 0; i < NV; ++i) {
            float t = q[0][i] + q[1][i];
            t += __shfl_xor(t, 1, 64);
            q[0][i] = t;
          }
          const int ly = (oy0 >> 1) + wpx, lx = (ox0 >> 1) + (rho >> 1);
          if ((rho & 1) == 0 && ly < Hl && lx < Wl && c0 < a.c1_out) {
            T* dst = out + ((size_t)(b * Hl + ly) * Wl + lx) * (size_t)a.c1_out + c0;
            if (G::MT == 2) {
              float v8[8];
#pragma unroll
              for (int i = 0; i < 8; ++i) v8[i] = q[0][i & 7];
              ffa_store8<T>(dst, v8);
            } else {
#pragma unroll
              for (int i = 0; i < 4; ++i) ffa_store_elem<T>(dst + i, q[0][i]);
            }
          }
        } else {  // 16x16 tiles: fragment nt = rows 4*wpx + 2*nt + (rho >> 4), lane & 15 = column
#pragma unroll
          for (int nt = 0; nt < G::NT; ++nt) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
              float t = q[nt][i] + __shfl_xor(q[nt][i], 16, 64);
              t += __shfl_xor(t, 1, 64);
              q[nt][i] = t;
            }
            const int ly = (oy0 >> 1) + 2 * wpx + nt, lx = (ox0 >> 1) + ((rho & 15) >> 1);
            if ((rho & 17) == 0 && ly < Hl && lx < Wl && c0 < a.c1_out) {
              T* dst = out + ((size_t)(b * Hl + ly) * Wl + lx) * (size_t)a.c1_out + c0;
              if (G::MT == 2) {
                float v8[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) v8[i] = q[nt][i & 7];
                ffa_store8<T>(dst, v8);
              } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) ffa_store_elem<T>(dst + i, q[nt][i]);
              }
            }
          }
        }
      }
      return;
    }
  }
  // BatchNorm batch statistics of the tensor being written, from the registers that hold it (a.stats != null):
  // per lane NCH channels x (sum, sum of squares) over its pixels, of the values AS STORED (bf16-rounded)
  constexpr int NCH = (G::MT == 2) ? 32 : 16;
  float st[2 * NCH];
  const bool want_stats = a.stats != nullptr;
#pragma unroll
  for (int i = 0; i < 2 * NCH; ++i) st[i] = 0.f;
#pragma unroll
  for (int nt = 0; nt < G::NT; ++nt) {
    const int n = wpx * G::WAVE_PX + nt * 32 + rho;
    const int oy = oy0 + n / TW, ox = ox0 + n % TW;
    if (oy >= a.Ho || ox >= a.Wo) continue;
    const long long pix = ((long long)(b * a.Ho + oy) * a.Wo + ox) * (long long)opitch - cshift;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (G::MT == 2) {
        const int c0 = co_wave + 16 * g + 8 * half;
        if (c0 >= a.Co) continue;
        float v[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          v[i] = acc[0][nt][4 * g + i];
          v[4 + i] = acc[G::MT - 1][nt][4 * g + i];
        }
        if (a.bias) {
#pragma unroll
          for (int i = 0; i < 8; ++i) v[i] += a.bias[c0 + i];
        }
        if (res) {
          float rv[8];
          ffa_load8<T>(res + pix + c0, rv);
#pragma unroll
          for (int i = 0; i < 8; ++i) v[i] += rv[i];
        }
        if (a.relu) {
#pragma unroll
          for (int i = 0; i < 8; ++i) v[i] = fmaxf(v[i], 0.f);
        }
        ffa_store8<T>(out + pix + c0, v);
        if (want_stats) {
          if (a.bnx) {
            float xv[8], sc[8], sh[8];
            ffa_load8<T>(static_cast<const T*>(a.bnx) + pix + c0, xv);
            ffa_load8<float>(a.bn_sc + c0, sc);
            ffa_load8<float>(a.bn_sh + c0, sh);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              const float r = (EB == 2) ? ffa_bf16_bits_to_f32(ffa_f32_to_bf16_bits(v[i])) : v[i];
              const float gg = (xv[i] * sc[i] + sh[i]) > 0.f ? r : 0.f;  // same fma as the forward / apply kernels
              st[g * 8 + i] += gg;
              st[NCH + g * 8 + i] = __builtin_fmaf(gg, xv[i], st[NCH + g * 8 + i]);
            }
          } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              const float r = (EB == 2) ? ffa_bf16_bits_to_f32(ffa_f32_to_bf16_bits(v[i])) : v[i];
              st[g * 8 + i] += r;
              st[NCH + g * 8 + i] = __builtin_fmaf(r, r, st[NCH + g * 8 + i]);  // explicit: both conv kernels must round alike
            }
          }
        }
      } else {
        const int c0 = co_wave + 8 * g + 4 * half;
        if (c0 >= a.Co) continue;
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = acc[0][nt][4 * g + i];
        if (a.bias) {
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] += a.bias[c0 + i];
        }
        if (res) {
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] += ffa_load_elem<T>(res + pix + c0 + i);
        }
        if (a.relu) {
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], 0.f);
        }
        if (EB == 2) {
          uint2 u;
          u.x = ffa_pack_bf16x2(v[0], v[1]);
          u.y = ffa_pack_bf16x2(v[2], v[3]);
          *reinterpret_cast<uint2*>(out + pix + c0) = u;
        } else {
          *reinterpret_cast<float4*>(out + pix + c0) = make_float4(v[0], v[1], v[2], v[3]);
        }
        if (want_stats) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float r = (EB == 2) ? ffa_bf16_bits_to_f32(ffa_f32_to_bf16_bits(v[i])) : v[i];
            if (a.bnx) {
              const float xi = ffa_load_elem<T>(static_cast<const T*>(a.bnx) + pix + c0 + i);
              const float gg = (xi * a.bn_sc[c0 + i] + a.bn_sh[c0 + i]) > 0.f ? r : 0.f;
              st[g * 4 + i] += gg;
              st[NCH + g * 4 + i] = __builtin_fmaf(gg, xi, st[NCH + g * 4 + i]);
            } else {
              st[g * 4 + i] += r;
              st[NCH + g * 4 + i] = __builtin_fmaf(r, r, st[NCH + g * 4 + i]);
            }
          }
        }
      }
    }
  }
  if (want_stats) {
    static_assert(WCO == 1, "the statistics epilogue assumes one co wave group per block");
    // Transposing reduction over the 32 lanes of a half-wave: at every step a lane keeps one half of its values and
    // adds the partner's copy of that half -- 2*NCH - 2 shuffles instead of 5 per value.  Afterwards lane rho holds
    // two entries of [sums | sums of squares]: entry index = (bits of rho, high to low) * 2 + j.
#pragma unroll
    for (int bit = 4; bit >= 0; --bit) {
      const int n = (2 * NCH) >> (4 - bit);  // values a lane still holds (compile-time: the loop is unrolled)
      if (n > 2) {
        const bool up = (rho >> bit) & 1;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
          if (j < n / 2) {
            // (the two reads go through an opaque asm: hipcc otherwise rewrites "up ? st[a] : st[b]" into
            // st[up ? a : b], a dynamically indexed register array = a 32-way compare/select chain per value)
            float lo = st[j], hi = st[j + n / 2];
            asm volatile("" : "+v"(lo), "+v"(hi));
            const float keep = up ? hi : lo;
            const float send = up ? lo : hi;
            st[j] = keep + __shfl_xor(send, 1 << bit, 64);
          }
        }
      } else {  // NCH == 16: the last lane bit is a plain butterfly, both lanes of a pair end up with the totals
        st[0] += __shfl_xor(st[0], 1 << bit, 64);
        st[1] += __shfl_xor(st[1], 1 << bit, 64);
      }
    }
    // the pixel waves of the block add up through LDS (free: a barrier followed the last fragment reads)
    float* red = reinterpret_cast<float*>(smem);
    red[(wpx * 64 + lane) * 2 + 0] = st[0];
    red[(wpx * 64 + lane) * 2 + 1] = st[1];
    __syncthreads();
    constexpr int NOUT = (G::MT == 2) ? 128 : 64;
    if (tid < NOUT) {
      const int j = tid & 1;
      const int ln = (G::MT == 2) ? (tid >> 1) : ((tid >> 1) * 2);  // MT == 1: even lanes carry the totals
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < WPX; ++w) t += red[(w * 64 + ln) * 2 + j];
      const int r5 = ln & 31, hf = ln >> 5;
      const int which = r5 >> 4;
      int c;
      if (G::MT == 2) {
        const int L = (r5 & 15) * 2 + j;
        c = cb * BCO + 16 * (L >> 3) + 8 * hf + (L & 7);
      } else {
        const int L = ((r5 >> 1) & 7) * 2 + j;
        c = cb * BCO + 8 * (L >> 2) + 4 * hf + (L & 3);
      }
      if (c < a.Co) a.stats[((size_t)pt * 2 + which) * a.Co + c] = t;
    }
  }
  FFA_TRACE(7)
}

// ------------------------------------------------------------------------------------------------
// Persistent variant of the pipelined 3x3 stride-1 path (the default for plain input, dil 1, no split / bnbwd
// epilogue; FFA_CONV_PERSIST=0 disables).  A block walks the virtual block list with stride gridDim.x and carries the software pipeline ACROSS
// tiles: the next tile's halo and first two weight slabs are requested from inside the last chunk group of the
// current tile and stored to LDS before the current tile's epilogue, so the prologue burst (35-40 % of a block's
// life on the short-K layers, tools/conv_trace.py) and the epilogue's stores overlap matrix work instead of
// standing alone.  The statistics epilogue reduces through its own 2 KB of LDS (the halo image already belongs to
// the next tile by then).
template <typename T, int BCO, int TH, int TW, int HK>
__global__ void __launch_bounds__(256, 2) conv3x3_persist_kernel(ConvArgs a) {
  constexpr int KW = 3;
  using G = ConvGeom<3, 3, 1, 3, BCO, 1, 4, TH, TW, HK>;
  constexpr int EB = ElemTraits<T>::kBytes;
  constexpr int WPX = 4;
  __shared__ __align__(16) unsigned char smem[G::LDS_BYTES + 2048];
  unsigned char* sIn = smem;
  unsigned char* sW = smem + G::HALO_BYTES;
  float* red = reinterpret_cast<float*>(smem + G::LDS_BYTES);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wpx = tid >> 6;
  const int rho = lane & 31;
  const int half = lane >> 5;
  const int total_vb = ((a.npt + 7) / 8) * 8 * a.ncb;
  const int total_chunks = a.nchunks;
  const size_t slab = (size_t)(BCO * G::TAPS * 32);

  int aoff[G::MT];
#pragma unroll
  for (int mt = 0; mt < G::MT; ++mt) aoff[mt] = (mt * 32 + rho) * G::WP + half * 16;
  int boff[G::NT];
#pragma unroll
  for (int nt = 0; nt < G::NT; ++nt) {
    const int n = wpx * G::WAVE_PX + nt * 32 + rho;
    boff[nt] = ((n / TW) * G::IW + (n % TW)) * G::PP + half * 16;
  }
  // LDS address of halo piece k of this thread: piece tid + k * NTHR is pixel tid / HPP + k * (NTHR / HPP)
  static_assert(G::NTHR % G::HPP == 0, "halo pieces of one thread share the 16-byte slot");
  const int hlds0 = (tid / G::HPP) * G::PP + (tid % G::HPP) * 16;
  constexpr int HLDS_STEP = (G::NTHR / G::HPP) * G::PP;

  struct TileId {
    int pt, cb, b, oy0, ox0;
  };
  // virtual block -> tile (same XCD-aware order as conv_igemm_kernel); pt >= npt marks the padding of the last group
  auto decode = [&](int vb) {
    TileId t;
    const int j = vb >> 3;
    t.pt = (j / a.ncb) * 8 + (vb & 7);
    t.cb = j % a.ncb;
    const int tx = t.pt % a.tiles_x;
    const int t2 = t.pt / a.tiles_x;
    t.b = t2 / a.tiles_y;
    t.oy0 = (t2 % a.tiles_y) * TH;
    t.ox0 = tx * TW;
    return t;
  };
  auto next_valid = [&](int vb) {
    while (vb < total_vb && decode(vb).pt >= a.npt) vb += gridDim.x;
    return vb;
  };
  auto halo_offsets = [&](const TileId& t, int* ho) {
#pragma unroll
    for (int k = 0; k < G::NHP; ++k) {
      const int i = tid + k * G::NTHR;
      const int q = i / G::HPP, hh = i % G::HPP;
      const int vy = t.oy0 - a.pad + q / G::IW;
      const int vx = t.ox0 - a.pad + q % G::IW;
      const bool ok = (i < G::H_PIECES) && vy >= 0 && vx >= 0 && vy < a.Hi && vx < a.Wi;
      ho[k] = ok ? (((t.b * a.Hi + vy) * a.Wi + vx) * a.Ci * EB + hh * 16) : -1;
    }
  };

  int vb = next_valid(blockIdx.x);
  if (vb >= total_vb) return;
  TileId cur = decode(vb);
  int hoff[G::NHP];  // piece offsets of the NEXT halo fill (this tile's next group, then the next tile's first)
  halo_offsets(cur, hoff);
  const unsigned char* in_b = static_cast<const unsigned char*>(a.in);
  const unsigned char* w_all = static_cast<const unsigned char*>(a.w);
  const unsigned char* w_b = w_all + (size_t)cur.cb * total_chunks * slab;

  ffa_u32x4 wregA[G::NWP], wregB[G::NWP];
  ffa_u32x4 hreg[G::NHP];
  ffa_f32x16 acc[G::MT][G::NT];

#define FFA_P_STORE_W(WR)                                                                  \
  {                                                                                        \
    _Pragma("unroll") for (int k = 0; k < G::NWP; ++k) {                                   \
      const int i = tid + k * G::NTHR;                                                     \
      if (k + 1 < G::NWP || G::W_PIECES % G::NTHR == 0 || i < G::W_PIECES) {               \
        const int row = i / (G::TAPS * 2), col = i % (G::TAPS * 2);                        \
        *reinterpret_cast<ffa_u32x4*>(sW + row * G::WP + col * 16) = WR[k];                \
      }                                                                                    \
    }                                                                                      \
  }
#define FFA_P_STORE_H(HO)                                                                  \
  {                                                                                        \
    _Pragma("unroll") for (int k = 0; k < G::NHP; ++k) {                                   \
      const int i = tid + k * G::NTHR;                                                     \
      if (k + 1 < G::NHP || G::H_PIECES % G::NTHR == 0 || i < G::H_PIECES)                 \
        *reinterpret_cast<ffa_u32x4*>(sIn + hlds0 + k * HLDS_STEP) = (HO[k] >= 0) ? hreg[k] : ffa_u32x4{0u, 0u, 0u, 0u}; \
    }                                                                                      \
  }

  // prologue of the block's first tile (the only exposed one)
  {
    const ffa_u32x4* wsrc = reinterpret_cast<const ffa_u32x4*>(w_b);
#pragma unroll
    for (int k = 0; k < G::NWP; ++k) {
      const int i = tid + k * G::NTHR;
      wregA[k] = wsrc[(k + 1 < G::NWP || G::W_PIECES % G::NTHR == 0 || i < G::W_PIECES) ? i : 0];
    }
#pragma unroll
    for (int k = 0; k < G::NHP; ++k) hreg[k] = *reinterpret_cast<const ffa_u32x4*>(in_b + (unsigned)(hoff[k] >= 0 ? hoff[k] : 0));
    FFA_P_STORE_W(wregA)
    FFA_P_STORE_H(hoff)
    __syncthreads();
    const ffa_u32x4* wsrc1 = reinterpret_cast<const ffa_u32x4*>(w_b + slab);
#pragma unroll
    for (int k = 0; k < G::NWP; ++k) {
      const int i = tid + k * G::NTHR;
      wregA[k] = wsrc1[(k + 1 < G::NWP || G::W_PIECES % G::NTHR == 0 || i < G::W_PIECES) ? i : 0];
    }
  }

  constexpr int HJ = (HK >= 4) ? 1 : 0;
  while (true) {
    const int nvb = next_valid(vb + gridDim.x);
    const bool has_next = nvb < total_vb;
    const TileId nxt = decode(has_next ? nvb : vb);
    const unsigned char* w_n = w_all + (size_t)nxt.cb * total_chunks * slab;

#pragma unroll
    for (int mt = 0; mt < G::MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < G::NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

    for (int c0 = 0; c0 < total_chunks; c0 += HK) {
      const bool last_group = (c0 + HK >= total_chunks);
      const bool cross = last_group && has_next;  // the halo requested during this group belongs to the next tile
      // next halo fill: the following channel group of this tile, or group 0 of the next tile; a block without a
      // next tile re-reads its last group (never stored)
      const unsigned char* hbase = in_b + (last_group ? (has_next ? 0 : c0 * 32) : (c0 + HK) * 32);
      // from here on this tile needs no further halo of its own: hoff switches to the next tile
      if (cross) halo_offsets(nxt, hoff);
#pragma unroll
      for (int j = 0; j < HK; ++j) {
        const int c = c0 + j;
        // weight slab two chunks ahead; past the end of this tile it is chunk 0 / 1 of the next tile's co block
        const unsigned char* wp = (c + 2 < total_chunks) ? w_b + (size_t)(c + 2) * slab
                                  : (has_next ? w_n + (size_t)(c + 2 - total_chunks) * slab
                                              : w_b + (size_t)(total_chunks - 1) * slab);
        const ffa_u32x4* wsrc = reinterpret_cast<const ffa_u32x4*>(wp);
        auto issue = [&](int tap) __attribute__((always_inline)) {
#pragma unroll
          for (int k = 0; k < G::NWP; ++k) {
            if (k % G::TAPS != tap) continue;
            const int i = tid + k * G::NTHR;
            const ffa_u32x4 v = wsrc[(k + 1 < G::NWP || G::W_PIECES % G::NTHR == 0 || i < G::W_PIECES) ? i : 0];
            if (j & 1) wregA[k] = v;
            else wregB[k] = v;
          }
          if (j == HJ) {
#pragma unroll
            for (int k = 0; k < G::NHP; ++k) {
              if (k % G::TAPS != tap) continue;
              hreg[k] = *reinterpret_cast<const ffa_u32x4*>(hbase + (unsigned)(hoff[k] >= 0 ? hoff[k] : 0));
            }
          }
        };
        // ---- one chunk of matrix work (same pinned MFMA / ds_read / global_load interleave as conv_igemm_kernel)
        {
          const int sub = j * 32;
          ffa_u32x4 af[2][G::MT], bf[2][G::NT];
#pragma unroll
          for (int mt = 0; mt < G::MT; ++mt) af[0][mt] = *reinterpret_cast<const ffa_u32x4*>(sW + aoff[mt]);
#pragma unroll
          for (int nt = 0; nt < G::NT; ++nt) bf[0][nt] = *reinterpret_cast<const ffa_u32x4*>(sIn + boff[nt] + sub);
#pragma unroll
          for (int tap = 0; tap < G::TAPS; ++tap) {
            const int cu = tap & 1, nx = cu ^ 1;
            __builtin_amdgcn_sched_barrier(0);
            issue(tap);
            if (tap + 1 < G::TAPS) {
              const int r1 = (tap + 1) / KW, s1 = (tap + 1) % KW;
#pragma unroll
              for (int mt = 0; mt < G::MT; ++mt)
                af[nx][mt] = *reinterpret_cast<const ffa_u32x4*>(sW + aoff[mt] + (tap + 1) * 32);
#pragma unroll
              for (int nt = 0; nt < G::NT; ++nt)
                bf[nx][nt] = *reinterpret_cast<const ffa_u32x4*>(sIn + boff[nt] + sub + (r1 * G::IW + s1) * G::PP);
            }
#pragma unroll
            for (int mt = 0; mt < G::MT; ++mt)
#pragma unroll
              for (int nt = 0; nt < G::NT; ++nt) Mma<T>::run(af[cu][mt], bf[cu][nt], acc[mt][nt]);
            {
              constexpr int NM = G::MT * G::NT;
              const int NR = (tap + 1 < G::TAPS) ? G::MT + G::NT : 0;
              int NV = 0;
#pragma unroll
              for (int k = 0; k < G::NWP; ++k) NV += (k % G::TAPS == tap) ? 1 : 0;
              if (j == HJ) {
#pragma unroll
                for (int k = 0; k < G::NHP; ++k) NV += (k % G::TAPS == tap) ? 1 : 0;
              }
              constexpr int PER = (sizeof(T) == 2) ? 1 : 4;
#pragma unroll
              for (int i = 0; i < NM; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, PER, 0);
                if (i < NR) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                if (i < NV) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
              }
#pragma unroll
              for (int i = NM; i < G::MT + G::NT; ++i)
                if (i < NR) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#pragma unroll
              for (int i = NM; i < NM + 4; ++i)
                if (i < NV) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        if (c + 1 < total_chunks || has_next) {
          if (j & 1) FFA_P_STORE_W(wregB)
          else FFA_P_STORE_W(wregA)
          if (j == HK - 1) FFA_P_STORE_H(hoff)
          __syncthreads();
        }
      }
    }

    // ---- epilogue of `cur` (its LDS images already hold the next tile) ----
    {
      T* out = static_cast<T*>(a.out);
      const T* res = static_cast<const T*>(a.res);
      const int co_wave = cur.cb * BCO;
      constexpr int NCH = (G::MT == 2) ? 32 : 16;
      float st[2 * NCH];
      const bool want_stats = a.stats != nullptr;
#pragma unroll
      for (int i = 0; i < 2 * NCH; ++i) st[i] = 0.f;
#pragma unroll
      for (int nt = 0; nt < G::NT; ++nt) {
        const int n = wpx * G::WAVE_PX + nt * 32 + rho;
        const int oy = cur.oy0 + n / TW, ox = cur.ox0 + n % TW;
        if (oy >= a.Ho || ox >= a.Wo) continue;
        const long long pix = ((long long)(cur.b * a.Ho + oy) * a.Wo + ox) * (long long)a.Co;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          if (G::MT == 2) {
            const int c0 = co_wave + 16 * g + 8 * half;
            if (c0 >= a.Co) continue;
            float v[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              v[i] = acc[0][nt][4 * g + i];
              v[4 + i] = acc[G::MT - 1][nt][4 * g + i];
            }
            if (a.bias) {
#pragma unroll
              for (int i = 0; i < 8; ++i) v[i] += a.bias[c0 + i];
            }
            if (res) {
              float rv[8];
              ffa_load8<T>(res + pix + c0, rv);
#pragma unroll
              for (int i = 0; i < 8; ++i) v[i] += rv[i];
            }
            if (a.relu) {
#pragma unroll
              for (int i = 0; i < 8; ++i) v[i] = fmaxf(v[i], 0.f);
            }
            ffa_store8<T>(out + pix + c0, v);
            if (want_stats) {
#pragma unroll
              for (int i = 0; i < 8; ++i) {
                const float r = (EB == 2) ? ffa_bf16_bits_to_f32(ffa_f32_to_bf16_bits(v[i])) : v[i];
                st[g * 8 + i] += r;
                st[NCH + g * 8 + i] = __builtin_fmaf(r, r, st[NCH + g * 8 + i]);  // explicit: both conv kernels must round alike
              }
            }
          } else {
            const int c0 = co_wave + 8 * g + 4 * half;
            if (c0 >= a.Co) continue;
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = acc[0][nt][4 * g + i];
            if (a.bias) {
#pragma unroll
              for (int i = 0; i < 4; ++i) v[i] += a.bias[c0 + i];
            }
            if (res) {
#pragma unroll
              for (int i = 0; i < 4; ++i) v[i] += ffa_load_elem<T>(res + pix + c0 + i);
            }
            if (a.relu) {
#pragma unroll
              for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], 0.f);
            }
            if (EB == 2) {
              uint2 u;
              u.x = ffa_pack_bf16x2(v[0], v[1]);
              u.y = ffa_pack_bf16x2(v[2], v[3]);
              *reinterpret_cast<uint2*>(out + pix + c0) = u;
            } else {
              *reinterpret_cast<float4*>(out + pix + c0) = make_float4(v[0], v[1], v[2], v[3]);
            }
            if (want_stats) {
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const float r = (EB == 2) ? ffa_bf16_bits_to_f32(ffa_f32_to_bf16_bits(v[i])) : v[i];
                st[g * 4 + i] += r;
                st[NCH + g * 4 + i] = __builtin_fmaf(r, r, st[NCH + g * 4 + i]);
              }
            }
          }
        }
      }
      if (want_stats) {  // same transposing reduction and channel map as conv_igemm_kernel
#pragma unroll
        for (int bit = 4; bit >= 0; --bit) {
          const int n = (2 * NCH) >> (4 - bit);
          if (n > 2) {
            const bool up = (rho >> bit) & 1;
#pragma unroll
            for (int jj = 0; jj < NCH; ++jj) {
              if (jj < n / 2) {
                float lo = st[jj], hi = st[jj + n / 2];
                asm volatile("" : "+v"(lo), "+v"(hi));
                const float keep = up ? hi : lo;
                const float send = up ? lo : hi;
                st[jj] = keep + __shfl_xor(send, 1 << bit, 64);
              }
            }
          } else {
            st[0] += __shfl_xor(st[0], 1 << bit, 64);
            st[1] += __shfl_xor(st[1], 1 << bit, 64);
          }
        }
        red[(wpx * 64 + lane) * 2 + 0] = st[0];
        red[(wpx * 64 + lane) * 2 + 1] = st[1];
        __syncthreads();
        constexpr int NOUT = (G::MT == 2) ? 128 : 64;
        if (tid < NOUT) {
          const int jj = tid & 1;
          const int ln = (G::MT == 2) ? (tid >> 1) : ((tid >> 1) * 2);
          float t = 0.f;
#pragma unroll
          for (int w = 0; w < WPX; ++w) t += red[(w * 64 + ln) * 2 + jj];
          const int r5 = ln & 31, hf = ln >> 5;
          const int which = r5 >> 4;
          int c;
          if (G::MT == 2) {
            const int L = (r5 & 15) * 2 + jj;
            c = cur.cb * BCO + 16 * (L >> 3) + 8 * hf + (L & 7);
          } else {
            const int L = ((r5 >> 1) & 7) * 2 + jj;
            c = cur.cb * BCO + 8 * (L >> 2) + 4 * hf + (L & 3);
          }
          if (c < a.Co) a.stats[((size_t)cur.pt * 2 + which) * a.Co + c] = t;
        }
        __syncthreads();  // red is reused by the next tile
      }
    }
    if (!has_next) break;
    vb = nvb;
    cur = nxt;
    w_b = w_n;
  }
#undef FFA_P_STORE_W
#undef FFA_P_STORE_H
}

// ------------------------------------------------------------------------------------------------
// host side: configuration choice + launch

static int conv_rg(int kh) { return kh == 7 ? 1 : kh; }

// Preferred block height in output channels for a layer with `cout` real output channels.  The
// caller packs the weights with this value and hands the same value back in ffa_conv_call_t.
static int conv_pref_bco(int kh, int kw, int stride, int cout) {
  // 64 rows + deep (full 128-byte line) halo staging beats 128 rows + 32-byte staging, see ConvGeom
  if (kh == 3 && kw == 3 && stride == 1) return cout > 32 ? 64 : 32;
  return cout > 32 ? 64 : 32;
}

static bool conv_supported(int kh, int kw, int stride, int bco) {
  const bool shape = (kh == 3 && kw == 3 && (stride == 1 || stride == 2)) ||
                     (kh == 1 && kw == 1 && (stride == 1 || stride == 2)) || (kh == 7 && kw == 7 && stride == 2);
  if (!shape) return false;
  return bco == 64 || bco == 32;
}

// Grid of the persistent 3x3 stride-1 kernel for a launch that would otherwise take `grid` one-tile blocks, or 0 for
// the one-tile kernel.  On by default for every eligible launch (same-box A/B: 15.79 -> 15.50 ms per training step,
// -4...-9 % on the 64-channel 128^2 / 256^2 layers whose grids need several dispatch rounds; a grid that fits one
// round simply runs one tile per block).  FFA_CONV_PERSIST=0 restores conv_igemm_kernel everywhere;
// FFA_CONV_PERSIST_MIN / FFA_CONV_PERSIST_GRID move the threshold / the grid (the tests force several tiles per
// block on small tensors).  Read per call: a getenv is noise next to a launch.
static int conv_persist_grid(int dil, int c1_out, const void* bnx, int grid) {
  const char* pe = getenv("FFA_CONV_PERSIST");
  if ((pe && pe[0] == '0') || dil != 1 || c1_out != 0 || bnx != nullptr) return 0;
  const char* pm = getenv("FFA_CONV_PERSIST_MIN");
  const char* pg = getenv("FFA_CONV_PERSIST_GRID");
  const int min_grid = pm ? atoi(pm) : 0;
  int pgrid = pg ? atoi(pg) : 512;
  pgrid = pgrid < 8 ? 8 : (pgrid / 8) * 8;  // whole groups of 8: a block keeps its XCD across tiles
  if (grid <= min_grid) return 0;
  return pgrid < grid ? pgrid : grid;
}

// The route (ffa_igemm_route) has chosen kernel, halo depth, tile and grid; the launch chain only turns them into
// template arguments.
template <typename T, int KH, int KW, int STRIDE, int RG, int BCO, int WCO, int WPX, int TH, int TW, int HK,
          bool UP = false>
static int launch_hk(const ConvArgs& a, const ffa_conv_route_t& r, hipStream_t stream) {
  if (r.kernel == FFA_CONV_KERNEL_PERSIST) {
    if constexpr (KH == 3 && KW == 3 && STRIDE == 1 && HK >= 2 && !UP && WCO == 1 && WPX == 4) {
      hipLaunchKernelGGL((conv3x3_persist_kernel<T, BCO, TH, TW, HK>), dim3(r.grid), dim3(256), 0, stream, a);
      return ffa_check_launch("conv3x3_persist");
    }
    ffa_set_error("conv: routed to a persistent kernel that is not instantiated");
    return FFA_ERR_UNSUPPORTED;
  }
  hipLaunchKernelGGL((conv_igemm_kernel<T, KH, KW, STRIDE, RG, BCO, WCO, WPX, TH, TW, HK, UP>), dim3(r.grid),
                     dim3(64 * WCO * WPX), 0, stream, a);
  return ffa_check_launch("conv_igemm");
}

template <typename T, int KH, int KW, int STRIDE, int RG, int BCO, int WCO, int WPX, int TH, int TW>
static int launch_cfg(const ConvArgs& a, const ffa_conv_call_t& c, const ffa_conv_route_t& r, hipStream_t stream) {
  // deep halo staging for the 3x3 stride-1 workhorse when whole 64- / 128-byte runs of channels exist
  // (a 128-row block was measured equal at best: its weight slab leaves no LDS for the deep halo at two blocks
  // per CU, so 64 rows is the largest block instantiated)
  if constexpr (KH == 3 && STRIDE == 1) {
    if (c.form == FFA_CONV_UPCAT) {  // two-source (nearest x2 + concat) loader: the route checked that C1 is whole groups
      if (r.variant == 4) return launch_hk<T, KH, KW, STRIDE, RG, BCO, WCO, WPX, TH, TW, 4, true>(a, r, stream);
      return launch_hk<T, KH, KW, STRIDE, RG, BCO, WCO, WPX, TH, TW, 2, true>(a, r, stream);
    }
    if (r.variant == 4) return launch_hk<T, KH, KW, STRIDE, RG, BCO, WCO, WPX, TH, TW, 4>(a, r, stream);
    if (r.variant == 2) return launch_hk<T, KH, KW, STRIDE, RG, BCO, WCO, WPX, TH, TW, 2>(a, r, stream);
  }
  return launch_hk<T, KH, KW, STRIDE, RG, BCO, WCO, WPX, TH, TW, 1>(a, r, stream);
}

template <typename T, int KH, int KW, int STRIDE, int RG>
static int launch_shape(const ConvArgs& a, const ffa_conv_call_t& c, const ffa_conv_route_t& r, hipStream_t stream) {
  const bool wide = (r.tw == 32);
#define FFA_CONV_CASE(BCO_, WCO_, WPX_)                                                      \
  if (c.bco == BCO_) {                                                                       \
    return wide ? launch_cfg<T, KH, KW, STRIDE, RG, BCO_, WCO_, WPX_, 8, 32>(a, c, r, stream)   \
                : launch_cfg<T, KH, KW, STRIDE, RG, BCO_, WCO_, WPX_, 16, 16>(a, c, r, stream); \
  }
  FFA_CONV_CASE(64, 1, 4)
  FFA_CONV_CASE(32, 1, 4)
#undef FFA_CONV_CASE
  ffa_set_error("conv: no kernel for bco=%d", c.bco);
  return FFA_ERR_UNSUPPORTED;
}

template <typename T>
static int launch_dtype(const ConvArgs& a, const ffa_conv_call_t& c, const ffa_conv_route_t& r, hipStream_t stream) {
  if (c.kh == 3 && c.kw == 3 && c.stride == 1) return launch_shape<T, 3, 3, 1, 3>(a, c, r, stream);
  if (c.kh == 3 && c.kw == 3 && c.stride == 2) return launch_shape<T, 3, 3, 2, 3>(a, c, r, stream);
  if (c.kh == 1 && c.kw == 1 && c.stride == 1) return launch_shape<T, 1, 1, 1, 1>(a, c, r, stream);
  if (c.kh == 1 && c.kw == 1 && c.stride == 2) return launch_shape<T, 1, 1, 2, 1>(a, c, r, stream);
  if (c.kh == 7 && c.kw == 7 && c.stride == 2) return launch_shape<T, 7, 7, 2, 1>(a, c, r, stream);
  ffa_set_error("conv: unsupported kernel %dx%d stride %d", c.kh, c.kw, c.stride);
  return FFA_ERR_UNSUPPORTED;
}

extern "C" int ffa_conv_block_co(int kh, int kw, int stride, int cout) {
  const int bco = conv_pref_bco(kh, kw, stride, cout);
  return conv_supported(kh, kw, stride, bco) ? bco : FFA_ERR_UNSUPPORTED;
}

// Operand layout + block height for a layer: the value to hand to ffa_pack_conv_weight / ffa_conv_call_t as `bco`.
// Bits 0..11 = rows per block (the padded row count is a multiple of it); FFA_BCO_RING set = the operand is packed
// for the ring kernels of conv3x3_ring.hip (3x3 stride 1 pad 1, >= 64 rows, whole 64-byte groups of input channels).
// Which forms of call a layout serves is the router's table (conv_call.cpp); the caller clears the bit otherwise.
//   bf16: conv3x3_ring16_kernel (v_mfma_f32_16x16x32_bf16, LDS-DMA weights AND halo) is the default since round 3 --
//         36 / 32.5 / 34.7 us on the 128 / 256 / 512-channel layers against 40 / 37.3 / 38 for conv3x3_persist_kernel
//         (same box); FFA_RING=0 restores the conv_igemm operands;
//   f32:  conv3x3_ring_kernel only with FFA_RING=1 (it equals the persist kernel).
// allow_ring bit 1 (value 2): the caller can also take FFA_BCO_THIN -- conv3x3_thin_kernel for bf16 layers with at most
// 32 stored input channels and 32 rows; rows per block 16 or 32.  FFA_THIN=0 disables.
extern "C" int ffa_conv_plan(int dtype, int kh, int kw, int stride, int cout, int ci_pitch, int allow_ring) {
  const int bco = ffa_conv_block_co(kh, kw, stride, cout);
  if (bco < 0) return bco;
  {
    // the ResNet stem (bit 2 of `allow`; FFA_STEM=0 keeps conv_igemm_kernel<7, 7, 2>)
    const char* t = getenv("FFA_STEM");
    if ((allow_ring & 4) && !(t && t[0] == '0') && ffa_stem_takes_layer(dtype, kh, kw, stride, cout, ci_pitch))
      return 64 | FFA_BCO_STEM;
  }
  {
    const char* t = getenv("FFA_THIN");
    if ((allow_ring & 2) && !(t && t[0] == '0') && ffa_thin_takes_layer(dtype, kh, kw, stride, cout, ci_pitch))
      return (cout <= 16 ? 16 : 32) | FFA_BCO_THIN | (ci_pitch == 32 ? FFA_BCO_THIN32 : 0);
  }
  allow_ring &= 1;
  const char* e = getenv("FFA_RING");
  const int eb = (dtype == FFA_BF16) ? 2 : 4;
  const bool on = (dtype == FFA_BF16) ? !(e && e[0] == '0') : (e && e[0] == '1');
  if (allow_ring && on && kh == 3 && kw == 3 && stride == 1 && cout >= 64 && (ci_pitch * eb) % 64 == 0)
    return 64 | FFA_BCO_RING;
  return bco;
}

extern "C" int ffa_conv_row_group(int kh) { return conv_rg(kh); }

// 32-byte channel groups staged per halo fill (HK of ConvGeom) for a convolution over Ci stored input channels
static int igemm_halo_groups(int dtype, int kh, int stride, int Ci) {
  const int nchunks = Ci * ffa_conv_elem_bytes(dtype) / 32;
  if (!(kh == 3 && stride == 1)) return 1;
  return nchunks % 4 == 0 ? 4 : (nchunks % 2 == 0 ? 2 : 1);
}

// The two-source loader fetches whole halo channel groups from one source: C1 must cover a whole number of them
bool ffa_igemm_upcat_split_ok(int dtype, int c1, int c2) {
  const int hk = igemm_halo_groups(dtype, 3, 1, c1 + c2);
  return hk > 1 && (c1 * ffa_conv_elem_bytes(dtype)) % (hk * 32) == 0;
}

// conv_igemm layout: every supported kernel shape in the plain form (dil 1 / 2, statistics, BatchNorm-backward
// partials), the two-source form when C1 covers whole channel groups, the pooled / split form when C1 is whole blocks.
int ffa_igemm_route(const ffa_conv_call_t& c, ffa_conv_route_t* r) {
  if (!conv_supported(c.kh, c.kw, c.stride, c.bco)) {
    ffa_set_error("conv: unsupported kernel %dx%d stride %d block %d", c.kh, c.kw, c.stride, c.bco);
    return FFA_ERR_UNSUPPORTED;
  }
  if (c.co_rows % c.bco != 0) {  // (an argument error in the plain form, as it always was)
    ffa_set_error("conv: packed weight rows %d not a multiple of block %d", c.co_rows, c.bco);
    return c.form == FFA_CONV_UPCAT ? FFA_ERR_UNSUPPORTED : FFA_ERR_ARG;
  }
  const int eb = ffa_conv_elem_bytes(c.dtype);
  r->variant = igemm_halo_groups(c.dtype, c.kh, c.stride, c.Ci);
  if (c.form == FFA_CONV_UPCAT) {
    const int c2 = c.Ci - c.c1;
    FFA_REQUIRE((long long)c.B * c.Hi * c.Wi * (c.c1 > c2 ? c.c1 : c2) * eb < (1LL << 31),
                "conv_upcat: source tensors must be smaller than 2 GiB (32-bit piece offsets)");
    if (!ffa_igemm_upcat_split_ok(c.dtype, c.c1, c2)) {
      ffa_set_error("conv_upcat: C1 = %d does not cover whole %d-byte channel groups", c.c1, r->variant * 32);
      return FFA_ERR_UNSUPPORTED;
    }
  }
  if (c.form == FFA_CONV_POOLED && c.c1 % c.bco != 0) {
    ffa_set_error("dgrad_upcat: C1 = %d is not a multiple of the %d-row block", c.c1, c.bco);
    return FFA_ERR_UNSUPPORTED;
  }
  r->tw = (c.Wo >= 32) ? 32 : 16;
  r->th = (c.Wo >= 32) ? 8 : 16;
  r->tiles_x = ffa_cdiv(c.Wo, r->tw);
  r->tiles_y = ffa_cdiv(c.Ho, r->th);
  const long long ntiles = (long long)c.B * r->tiles_x * r->tiles_y;
  r->ncb = c.co_rows / c.bco;
  FFA_REQUIRE((ntiles + 7) / 8 * 8 * r->ncb < (1LL << 31), "conv: bad dims");
  r->ntiles = (int)ntiles;
  r->kernel = FFA_CONV_KERNEL_IGEMM;
  r->grid = ffa_cdiv(r->ntiles, 8) * 8 * r->ncb;
  // the persistent kernel exists for the pipelined (deep-halo) one-source 3x3 stride-1 instantiations
  if (c.kh == 3 && c.kw == 3 && c.stride == 1 && r->variant >= 2 && c.form != FFA_CONV_UPCAT) {
    const int pgrid = conv_persist_grid(c.dil, c.form == FFA_CONV_POOLED ? c.c1 : 0, c.bnx, r->grid);
    if (pgrid > 0) {
      r->kernel = FFA_CONV_KERNEL_PERSIST;
      r->grid = pgrid;
    }
  }
  return 0;
}

int ffa_igemm_launch(const ffa_conv_call_t& c, const ffa_conv_route_t& r, hipStream_t stream) {
  const bool up = c.form == FFA_CONV_UPCAT, pooled = c.form == FFA_CONV_POOLED;
  ConvArgs a;
  a.in = c.in;
  a.w = c.w;
  a.out = c.out;
  a.bias = c.bias;
  a.stats = c.stats;
  a.in2 = up ? c.in2 : nullptr;
  a.c1_bytes = up ? c.c1 * ffa_conv_elem_bytes(c.dtype) : 0;
  a.out2 = pooled ? c.out2 : nullptr;
  a.c1_out = pooled ? c.c1 : 0;
  a.bnx = c.bnx;
  a.bn_sc = c.bn_scale;
  a.bn_sh = c.bn_shift;
  a.res = c.residual;
  a.B = c.B; a.Hi = c.Hi; a.Wi = c.Wi; a.Ci = c.Ci;
  a.Ho = c.Ho; a.Wo = c.Wo; a.Co = c.Co;
  a.pad = c.pad; a.dil = c.dil; a.relu = c.relu;
  a.nchunks = c.Ci * ffa_conv_elem_bytes(c.dtype) / 32;
  a.tiles_x = r.tiles_x;
  a.tiles_y = r.tiles_y;
  a.npt = r.ntiles;
  a.ncb = r.ncb;
  if (c.dtype == FFA_BF16) return launch_dtype<ffa_bf16>(a, c, r, stream);
  return launch_dtype<float>(a, c, r, stream);
}

#if FFA_CONV_TRACE
extern "C" int ffa_conv_trace_read(long long* host_dst, int n) {
  if (n > 64 * 256) n = 64 * 256;
  hipDeviceSynchronize();
  return (int)hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(ffa_conv_trace_buf), (size_t)n * sizeof(long long));
}
extern "C" int ffa_conv_trace_clear() {
  static long long zeros[64 * 256];
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(ffa_conv_trace_buf), zeros, sizeof(zeros));
}
#endif
