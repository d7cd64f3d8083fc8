// 3x3 stride-1 pad-1 convolution (forward and stride-1 dgrad) on MFMA for gfx950 -- the "ring" kernel.
//
// Replaces the cuDNN / ATen conv2d of the ResNet-34 BasicBlocks and U-Net decoder blocks reached through
// segmentation_models_pytorch from flair_hub/models/monotemp_model.py:68-92 (called at
// flair_hub/models/flair_model.py:376 and :417-419), for the layers with >= 64 output channels and whole 64-byte
// groups of input channels -- the MFMA-bound part of the step.
//
// What differs from conv_igemm.hip (which stays for strided / 1x1 / 7x7 / thin layers):
//   * the weight operand -- two thirds of the bytes a block stages -- never touches a VGPR: it is packed in global
//     memory as the exact LDS image and streamed by LDS-DMA (global_load_lds_dwordx4) into a 3-slot ring, one slot
//     per kernel row of a 64-byte channel chunk, two phases ahead of its use, tracked with a counted vmcnt;
//   * ONE barrier per phase (a phase = one kernel row x 64 bytes of channels = 6 k-steps of MFMA per wave) instead
//     of two per 32-byte k-step chunk;
//   * the input halo (one third of the bytes) keeps the register path -- zero padding, and optionally a fused
//     BatchNorm + ReLU of the producing layer (relu(x * sc[c] + sh[c]), "normalise on load"), are applied in
//     registers -- and is double-buffered in LDS, requested a whole chunk (three phases) before it is stored;
//   * blocks are persistent: the phase stream runs across pixel tiles, so a tile's epilogue overlaps the loads of
//     the next one.
//
// GEMM orientation as in conv_igemm.hip: D[co][pixel] = W[co][k] * X[k][pixel]; a wave owns 64 output channels x
// NT*32 pixels; lanes end up with runs of 8 consecutive channels of one pixel (16-byte NHWC stores).
//
// LDS images
//   ring slot [wco][tap s][k-step][64 rows in fragment order][32 B], the two 16-byte halves of a row swapped when
//             bit 3 of the row is set  -> conflict-free ds_read_b128, linear (lane-order) DMA destination
//   halo      [k-step plane][halo pixel][32 B], halves swapped when bit 3 of the pixel's x is set; plane stride
//             = 64 mod 128 bytes -> conflict-free ds_read_b128 for 32 pixels of a row and conflict-free ds_write_b128
#include "ffa_gfx950.h"
#include "conv_call.h"

#include <stdlib.h>

// Developer instrumentation (never built by flairhip/build.py; tools/ring_trace.py builds a second library with
// -DFFA_RING_TRACE=1): wave 0 of every block records its lifetime in shader cycles (s_memtime) and in 100 MHz
// real-time ticks (s_memrealtime: their ratio is the clock the chip really holds under this kernel), and the cycles
// it spent in the prologue, waiting at phase-end synchronisations and in tile epilogues.
#ifndef FFA_RING_TRACE
#define FFA_RING_TRACE 0
#endif
#ifndef FFA_RING_SCHED
#define FFA_RING_SCHED 0  // 1: one fragment read behind every MFMA (measured slower, kept for A/B builds)
#endif
#if FFA_RING_TRACE
__device__ long long ffa_ring_trace_buf[1024 * 8];
#define RT_NOW() ((long long)__builtin_readcyclecounter())
#define RT_ADD(acc_, t0_) acc_ += RT_NOW() - (t0_)
#else
#define RT_NOW() 0ll
#define RT_ADD(acc_, t0_)
#endif

struct Ring3Args {
  const void* in;
  const void* w;        // ring layout (f32) / ring16 layout (bf16) of conv_pack.hip
  void* out;
  const float* bias;    // [Co] or null
  float* stats;         // [npt][2][Co] per-tile channel sums / sums of squares of the stored output, or null
  const void* res;      // same layout as out, or null
  const float* pro_sc;  // PRO kernels: the input is relu(in * pro_sc[c] + pro_sh[c]), evaluated while staging
  const float* pro_sh;
  int B, H, W;          // stride 1, pad 1: output H x W
  int Ci, Co;           // stored channel pitches (elements)
  int relu;
  int nchunks;          // Ci * sizeof(T) / 64
  int tiles_x, tiles_y, npt, ncb;
  long long cb64_stride;  // bytes between the operands of consecutive 64-row groups
  unsigned m_ncb, m_tx, m_ty;  // ffa_udiv_magic multipliers of ncb, tiles_x, tiles_y (ring16: tile walk on the scalar unit)
};

template <int WCO, int WPX, int NT, int TH, int TW>
struct RingGeom {
  static constexpr int MT = 2;
  static constexpr int KS = 2;  // 32-byte k-steps per chunk
  static constexpr int NW = WCO * WPX;
  static constexpr int NTHR = 64 * NW;
  static constexpr int BCO = 64 * WCO;
  static constexpr int NPX = TH * TW;
  static constexpr int IH = TH + 2;
  static constexpr int IW = (TW == 32) ? 34 : 24;  // TW == 16: a fragment spans two rows, IW = 0 mod 8 keeps reads conflict-free
  static constexpr int PLANE_RAW = IH * IW * 32;
  static constexpr int PLANE = PLANE_RAW + ((64 - PLANE_RAW % 128) + 128) % 128;  // = 64 mod 128
  static constexpr int HBUF = KS * PLANE;
  static constexpr int SLAB64 = 3 * KS * 64 * 32;  // one kernel row of one 64-row group: 12 KB
  static constexpr int SLOT = WCO * SLAB64;
  static constexpr int NSLOT = 3;
  static constexpr int NWI = SLOT / 1024 / NW;  // DMA wave-instructions per wave per phase
  static constexpr int H_PIECES = IH * IW * 4;
  static constexpr int NHP = (H_PIECES + NTHR - 1) / NTHR;
  static constexpr int RING_OFF = 0;
  static constexpr int HALO_OFF = NSLOT * SLOT;
  // the statistics epilogue reduces through ring slot 2: a tile's last phase is always kernel row 2, and the next
  // DMA into that slot is only issued at the top of the next tile's first phase
  static constexpr int RED_OFF = RING_OFF + 2 * SLOT;
  static constexpr int RED_BYTES = NW * 64 * 2 * 4;
  static constexpr int LDS_BYTES = HALO_OFF + 2 * HBUF;
  static_assert(RED_BYTES <= SLOT, "statistics scratch must fit a ring slot");
  static_assert(NPX == WPX * NT * 32, "pixel tile must be covered by the pixel waves");
  static_assert(TW == 32 || TW == 16, "tile width");
  static_assert((SLOT / 1024) % NW == 0, "every wave issues the same number of DMA instructions");
  static_assert(PLANE % 128 == 64 && PLANE % 16 == 0, "plane stride");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

// phase-end synchronisation: this wave's DMA of the NEXT phase has landed when at most its newest NWI vector-memory
// operations (the DMA of the phase after that, issued at the top of this phase) are outstanding; its halo stores
// are in LDS (lgkmcnt); then the block meets: ffa_wait_vm_lgkm_barrier<NWI>, or ffa_wait_vm_barrier where no halo
// stores are pending, so that fragment reads requested for later steps stay in flight across the barrier.

template <typename T, int WCO, int WPX, int NT, int TH, int TW, int OCC, bool PRO>
__global__ void __launch_bounds__(64 * WCO * WPX, OCC) conv3x3_ring_kernel(Ring3Args a) {
  using G = RingGeom<WCO, WPX, NT, TH, TW>;
  constexpr int EB = ElemTraits<T>::kBytes;
  constexpr int EPF = ElemTraits<T>::kPerFrag;
  constexpr int MT = G::MT, KS = G::KS;
  __shared__ __align__(16) unsigned char smem[G::LDS_BYTES];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wco = wave / WPX;
  const int wpx = wave % WPX;
  const int rho = lane & 31;
  const int half = lane >> 5;
  const int NC = a.nchunks;
  const int PT = NC * 3;  // phases per tile
  const int total_vb = ((a.npt + 7) / 8) * 8 * a.ncb;

  // ---- per-lane LDS read addresses (everything else is an immediate) ----
  const int a0 = G::RING_OFF + wco * G::SLAB64 + rho * 32 + ((half ^ ((rho >> 3) & 1)) * 16);
  int bB[NT][3];  // includes the base of the CURRENT halo buffer
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int n = wpx * (NT * 32) + nt * 32 + rho;
    const int py = n / TW, px = n % TW;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const int hx = px + s;
      bB[nt][s] = G::HALO_OFF + (py * G::IW + hx) * 32 + ((half ^ ((hx >> 3) & 1)) * 16);
    }
  }

  // ---- halo staging geometry (tile independent part) ----
  static_assert(G::NTHR % 4 == 0, "a thread keeps its 16-byte slot of the 64-byte chunk");
  const int jj = tid & 3;  // piece of the 64-byte chunk: k-step jj >> 1, half jj & 1
  int hl[G::NHP];          // LDS byte offset inside a halo buffer
  int hyx[G::NHP];         // (hy << 16) | hx, or -1 past the last piece
#pragma unroll
  for (int k = 0; k < G::NHP; ++k) {
    const int q = (tid >> 2) + k * (G::NTHR / 4);
    const int hy = q / G::IW, hx = q % G::IW;
    hl[k] = (jj >> 1) * G::PLANE + q * 32 + (((jj & 1) ^ ((hx >> 3) & 1)) * 16);
    hyx[k] = (q < G::IH * G::IW) ? ((hy << 16) | hx) : -1;
  }

  struct TileId {
    int pt, cb, b, oy0, ox0;
  };
  auto decode = [&](int vb) {
    TileId t;
    const int j = vb >> 3;
    t.pt = (j / a.ncb) * 8 + (vb & 7);  // the co blocks of a pixel tile share an XCD's L2 (speed only)
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
  const int pix_bytes = a.Ci * EB;
  int hoff[G::NHP];  // byte offset of the piece from the input base (chunk 0), -1 = zero fill
  auto halo_offsets = [&](const TileId& t) {
#pragma unroll
    for (int k = 0; k < G::NHP; ++k) {
      const int hy = hyx[k] >> 16, hx = hyx[k] & 0xffff;
      const int vy = t.oy0 - 1 + hy, vx = t.ox0 - 1 + hx;
      const bool ok = hyx[k] >= 0 && vy >= 0 && vx >= 0 && vy < a.H && vx < a.W;
      hoff[k] = ok ? (((t.b * a.H + vy) * a.W + vx) * pix_bytes + jj * 16) : -1;
    }
  };

  const unsigned char* in_b = static_cast<const unsigned char*>(a.in);
  const unsigned char* w_all = static_cast<const unsigned char*>(a.w);

  ffa_u32x4 hreg[G::NHP];
  float psc[PRO ? EPF : 1], psh[PRO ? EPF : 1];

  // weight DMA of one phase: slab `ph` (chunk * 3 + kernel row) of co block `cb` -> ring slot `slot`
  auto issue_w = [&](int cb, int ph, int slot) {
#pragma unroll
    for (int i = 0; i < G::NWI; ++i) {
      const int ii = wave + i * G::NW;  // 1-KB piece of the slot (wave uniform)
      const int g64 = ii / (G::SLAB64 / 1024), pi = ii % (G::SLAB64 / 1024);
      const unsigned char* src = w_all + (long long)(cb * WCO + g64) * a.cb64_stride + (long long)ph * G::SLAB64 +
                                 pi * 1024 + lane * 16;
      ffa_lds_dma16(src, (unsigned)(size_t)(__attribute__((address_space(3))) void*)(smem + G::RING_OFF + slot * G::SLOT +
                                                                                  ii * 1024));
    }
  };
  // halo loads of one chunk (unconditional: a padding piece reads offset 0 and is zeroed when stored)
  auto load_h = [&](int chunk) {
    const unsigned char* base = in_b + chunk * 64;
#pragma unroll
    for (int k = 0; k < G::NHP; ++k)
      hreg[k] = *reinterpret_cast<const ffa_u32x4*>(base + (unsigned)(hoff[k] >= 0 ? hoff[k] : 0));
    if constexpr (PRO) {
      const int c0 = chunk * (64 / EB) + jj * EPF;
#pragma unroll
      for (int e = 0; e < EPF; ++e) {
        psc[e] = a.pro_sc[c0 + e];
        psh[e] = a.pro_sh[c0 + e];
      }
    }
  };
  auto store_h = [&](int buf) {
    unsigned char* dst = smem + G::HALO_OFF + buf * G::HBUF;
#pragma unroll
    for (int k = 0; k < G::NHP; ++k) {
      if (k + 1 < G::NHP || G::H_PIECES % G::NTHR == 0 || hyx[k] >= 0) {
        ffa_u32x4 v = hreg[k];
        if constexpr (PRO) {
          if constexpr (EB == 2) {
            float f[8];
            f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
            f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
            f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
            f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = fmaxf(__builtin_fmaf(f[e], psc[e], psh[e]), 0.f);
            v.x = ffa_pack_bf16x2(f[0], f[1]);
            v.y = ffa_pack_bf16x2(f[2], f[3]);
            v.z = ffa_pack_bf16x2(f[4], f[5]);
            v.w = ffa_pack_bf16x2(f[6], f[7]);
          } else {
            v.x = __float_as_uint(fmaxf(__builtin_fmaf(__uint_as_float(v.x), psc[0], psh[0]), 0.f));
            v.y = __float_as_uint(fmaxf(__builtin_fmaf(__uint_as_float(v.y), psc[1], psh[1]), 0.f));
            v.z = __float_as_uint(fmaxf(__builtin_fmaf(__uint_as_float(v.z), psc[2], psh[2]), 0.f));
            v.w = __float_as_uint(fmaxf(__builtin_fmaf(__uint_as_float(v.w), psc[3], psh[3]), 0.f));
          }
        }
        if (hoff[k] < 0) v = ffa_u32x4{0u, 0u, 0u, 0u};
        *reinterpret_cast<ffa_u32x4*>(dst + hl[k]) = v;
      }
    }
  };

  int vb = next_valid(blockIdx.x);
  if (vb >= total_vb) return;
  TileId cur = decode(vb);
#if FFA_RING_TRACE
  const long long rt_t0 = RT_NOW();
  const long long rt_r0 = (long long)__builtin_amdgcn_s_memrealtime();
  long long rt_sync = 0, rt_epi = 0, rt_pro = 0, rt_phases = 0;
#endif

  // ---- prologue of the block's first tile (the only exposed one) ----
  halo_offsets(cur);
  load_h(0);
  issue_w(cur.cb, 0, 0);
  issue_w(cur.cb, 1, 1);
  store_h(0);
  ffa_wait_vm_lgkm_barrier<0>();  // slabs 0 and 1 have landed, halo chunk 0 is stored
  RT_ADD(rt_pro, rt_t0);
  int hb = 0;  // halo buffer of the current chunk
  int hd = G::HBUF;  // byte distance from the current halo buffer to the other one

  // Fragment pipeline: the operands of MFMA step t+2 are requested while step t is multiplied (three register sets),
  // across phase, chunk and tile boundaries -- a wave alone on its SIMD keeps the matrix pipe fed through the LDS
  // latency, so the other block of the CU covers this block's epilogues instead of both crawling.  That needs the
  // next phase's LDS images visible two steps before a phase ends: the phase synchronisation sits in the MIDDLE of
  // a phase (behind step SYNC_AT), the weight DMA of phase p+2 is issued right behind it.
  constexpr int NST = 3 * KS;   // MFMA steps per phase: (tap s, k-step), 6
  constexpr int SYNC_AT = 2;
  static_assert(NST % 3 == 0, "the fragment set of a step is (step % 3) in every phase");
  ffa_u32x4 fa[3][MT], fb[3][NT];
  int bBn[NT];  // fragment base of tap 0 in the OTHER halo buffer (the next chunk's rows, read from kernel row 2)
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) bBn[nt] = bB[nt][0] + hd;
#pragma unroll
  for (int t = 0; t < 2; ++t) {  // steps 0 and 1 of the first phase
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      fa[t][mt] = *reinterpret_cast<const ffa_u32x4*>(smem + a0 + t * 2048 + mt * 1024);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      fb[t][nt] = *reinterpret_cast<const ffa_u32x4*>(smem + bB[nt][0] + t * G::PLANE);
  }

  ffa_f32x16 acc[MT][NT];

  while (true) {
    const int nvb = next_valid(vb + gridDim.x);
    const bool has_next = nvb < total_vb;
    const TileId nxt = decode(has_next ? nvb : vb);

#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

    for (int c = 0; c < NC; ++c) {
      // the halo requested during this chunk: the next chunk of this tile, or chunk 0 of the next tile
      const bool last_c = (c + 1 == NC);
      const bool hvalid = !last_c || has_next;
      if (last_c && has_next) halo_offsets(nxt);
      const int hchunk = last_c ? 0 : c + 1;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        // weight slab two phases ahead: this tile's, the next tile's first ones, or (no next tile) a re-read of
        // this tile's last slab, which lands in a slot nobody reads again (keeps every wave's DMA count uniform)
        int wcb_ = cur.cb, wph_ = c * 3 + r + 2;
        if (wph_ >= PT) {
          if (has_next) {
            wcb_ = nxt.cb;
            wph_ -= PT;
          } else {
            wph_ = PT - 1;
          }
        }
        const unsigned char* sA = smem + a0 + r * G::SLOT;
        const unsigned char* sAn = smem + a0 + ((r + 1) % 3) * G::SLOT;
#pragma unroll
        for (int st = 0; st < NST; ++st) {
          __builtin_amdgcn_sched_barrier(0);
          // ---- request the fragments of step st + 2 ----
          {
            const int t2 = st + 2, fbuf = t2 % 3;
            if (t2 < NST) {
              const int s1 = t2 / KS, k1 = t2 % KS;
#pragma unroll
              for (int mt = 0; mt < MT; ++mt)
                fa[fbuf][mt] = *reinterpret_cast<const ffa_u32x4*>(sA + t2 * 2048 + mt * 1024);
#pragma unroll
              for (int nt = 0; nt < NT; ++nt)
                fb[fbuf][nt] =
                    *reinterpret_cast<const ffa_u32x4*>(smem + bB[nt][s1] + k1 * G::PLANE + r * G::IW * 32);
            } else {  // steps 0 / 1 of the next phase: ring slot r + 1, halo row r + 1 (or row 0 of the next chunk)
              const int t3 = t2 - NST;
#pragma unroll
              for (int mt = 0; mt < MT; ++mt)
                fa[fbuf][mt] = *reinterpret_cast<const ffa_u32x4*>(sAn + t3 * 2048 + mt * 1024);
#pragma unroll
              for (int nt = 0; nt < NT; ++nt) {
                if (r < 2)
                  fb[fbuf][nt] = *reinterpret_cast<const ffa_u32x4*>(smem + bB[nt][0] + t3 * G::PLANE +
                                                                      (r + 1) * G::IW * 32);
                else
                  fb[fbuf][nt] = *reinterpret_cast<const ffa_u32x4*>(smem + bBn[nt] + t3 * G::PLANE);
              }
            }
          }
          // ---- multiply step st ----
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) Mma<T>::run(fa[st % 3][mt], fb[st % 3][nt], acc[mt][nt]);
          {
            constexpr int NM = MT * NT;
#if FFA_RING_SCHED == 0
            __builtin_amdgcn_sched_group_barrier(0x100, MT + NT, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, NM * Mma<T>::PER, 0);
#else
#pragma unroll
            for (int i = 0; i < NM; ++i) {
              __builtin_amdgcn_sched_group_barrier(0x008, Mma<T>::PER, 0);
              if (i < MT + NT) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
#endif
          }
          if (st == SYNC_AT) {
            __builtin_amdgcn_sched_barrier(0);
            // next chunk's halo into the other buffer (requested a whole chunk ago), then the phase meets: every
            // wave's DMA of the next phase has landed (issued a phase ago, so vmcnt(0) waits for nothing younger
            // than that), and every wave is done with the previous phase's ring slot -> refill it
            if (r == 2 && hvalid) store_h(hb ^ 1);
#if FFA_RING_TRACE
            const long long rt_s = RT_NOW();
            ++rt_phases;
#endif
            if (r == 2) ffa_wait_vm_lgkm_barrier<0>();  // halo stores must be in LDS
            else ffa_wait_vm_barrier<0>();
            RT_ADD(rt_sync, rt_s);
            issue_w(wcb_, wph_, (r + 2) % 3);
            if (r == 0 && hvalid) load_h(hchunk);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      // the next chunk reads the other halo buffer
      {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
          for (int s = 0; s < 3; ++s) bB[nt][s] += hd;
        }
        hb ^= 1;
        hd = -hd;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bBn[nt] = bB[nt][0] + hd;
      }
    }

    // ---- epilogue of `cur`: lane (rho, half) owns pixel n = wave px base + nt*32 + rho and, per g, 8 channels ----
#if FFA_RING_TRACE
    const long long rt_e = RT_NOW();
#endif
    {
      T* out = static_cast<T*>(a.out);
      const T* res = static_cast<const T*>(a.res);
      const int co_wave = cur.cb * G::BCO + wco * 64;
      constexpr int NCH = 32;
      float st[2 * NCH];
      const bool want_stats = a.stats != nullptr;
#pragma unroll
      for (int i = 0; i < 2 * NCH; ++i) st[i] = 0.f;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n = wpx * (NT * 32) + nt * 32 + rho;
        const int oy = cur.oy0 + n / TW, ox = cur.ox0 + n % TW;
        if (oy >= a.H || ox >= a.W) continue;
        const long long pix = ((long long)(cur.b * a.H + oy) * a.W + ox) * (long long)a.Co;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int c0 = co_wave + 16 * g + 8 * half;
          if (c0 >= a.Co) continue;
          float v[8];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            v[i] = acc[0][nt][4 * g + i];
            v[4 + i] = acc[1][nt][4 * g + i];
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
              const float rr = (EB == 2) ? ffa_bf16_bits_to_f32(ffa_f32_to_bf16_bits(v[i])) : v[i];
              st[g * 8 + i] += rr;
              st[NCH + g * 8 + i] = __builtin_fmaf(rr, rr, st[NCH + g * 8 + i]);  // explicit: all conv kernels round alike
            }
          }
        }
      }
      if (want_stats) {
        // transposing reduction over the 32 lanes of a half-wave (see conv_igemm.hip): afterwards lane rho holds two
        // entries of [sums | sums of squares], entry index = (bits of rho, high to low) * 2 + j
#pragma unroll
        for (int bit = 4; bit >= 0; --bit) {
          const int n = (2 * NCH) >> (4 - bit);
          const bool up = (rho >> bit) & 1;
#pragma unroll
          for (int j = 0; j < NCH; ++j) {
            if (j < n / 2) {
              float lo = st[j], hi = st[j + n / 2];
              asm volatile("" : "+v"(lo), "+v"(hi));
              const float keep = up ? hi : lo;
              const float send = up ? lo : hi;
              st[j] = keep + __shfl_xor(send, 1 << bit, 64);
            }
          }
        }
        float* red = reinterpret_cast<float*>(smem + G::RED_OFF);
        red[(wave * 64 + lane) * 2 + 0] = st[0];
        red[(wave * 64 + lane) * 2 + 1] = st[1];
        ffa_wait_lgkm_barrier();
        if (tid < 128 * WCO) {
          const int wc = tid >> 7, t7 = tid & 127;
          const int j = t7 & 1;
          const int ln = t7 >> 1;
          float t = 0.f;
#pragma unroll
          for (int w = 0; w < WPX; ++w) t += red[((wc * WPX + w) * 64 + ln) * 2 + j];
          const int r5 = ln & 31, hf = ln >> 5;
          const int which = r5 >> 4;
          const int L = (r5 & 15) * 2 + j;
          const int c = cur.cb * G::BCO + wc * 64 + 16 * (L >> 3) + 8 * hf + (L & 7);
          if (c < a.Co) a.stats[((size_t)cur.pt * 2 + which) * a.Co + c] = t;
        }
        ffa_wait_lgkm_barrier();  // red is reused by the next tile
      }
    }
    RT_ADD(rt_epi, rt_e);
    if (!has_next) break;
    vb = nvb;
    cur = nxt;
  }
#if FFA_RING_TRACE
  if (tid == 0 && blockIdx.x < 1024) {
    long long* o = ffa_ring_trace_buf + blockIdx.x * 8;
    o[0] = rt_t0;
    o[1] = RT_NOW();
    o[2] = rt_r0;
    o[3] = (long long)__builtin_amdgcn_s_memrealtime();
    o[4] = rt_sync;
    o[5] = rt_epi;
    o[6] = rt_pro;
    o[7] = rt_phases;
  }
#endif
  // the trailing DMA (re-reads of the last slab) must not outlive the block's LDS allocation
  ffa_wait_vm<0>();
}

// ------------------------------------------------------------------------------------------------
// bf16 on v_mfma_f32_16x16x32_bf16 ("ring16", round 3): the same ring / halo / phase structure with the 16x16 MFMA
// shape, whose K = 32 is one whole 64-byte channel chunk of one tap -- half the accumulator traffic per FLOP of the
// 32x32x16 form, and the shape on which the chip holds the higher clock under load (MI355X_MICROARCH.md, DVFS item 7).
//   * a wave owns 64 output channels x NT*16 pixels: MT = 4 tiles of 16 rows, NT pixel fragments of 16 columns;
//     accumulator tile (mt, nt): lane (col = lane & 15, kg = lane >> 4) holds rows 4*kg .. 4*kg+3 of pixel col.  The
//     pack stores output channel 16*kg + 4*mt + i of a 64-channel group in LDS row mt*16 + 4*kg + i, so a lane ends
//     up with 16 CONSECUTIVE channels of its pixel (two 16-byte NHWC stores);
//   * operand fragments: lane (row or pixel = lane & 15, kg) reads the 16 bytes of channels 8*kg .. 8*kg+7.  Both LDS
//     images are plain 64-byte rows (one chunk of one row / pixel) whose 16-byte slot index is XORed with 2 when bit 2
//     of the row index (weights) or of the halo column (pixels) is set: conflict-free ds_read_b128 for 16 consecutive
//     rows / pixels at ANY alignment (all 16 columns x 3 taps checked by enumeration), conflict-free ds_write_b128,
//     and still the linear destination LDS-DMA needs (the pack applies the XOR in global memory);
//   * a phase (kernel row r of one chunk) = 3 steps (taps) of MT*NT MFMAs; fragments of step t+1 are requested while
//     step t multiplies; the phase synchronisation sits behind step 0, the DMA of phase p+2 right behind it.

// source of the padding pieces of an LDS-DMA halo fill (per-lane source addresses: a border pixel reads zeros)

template <int WCO, int WPX, int NT, int TH, int TW>
struct Ring16Geom {
  static constexpr int MT = 4;
  static constexpr int NW = WCO * WPX;
  static constexpr int NTHR = 64 * NW;
  static constexpr int BCO = 64 * WCO;
  static constexpr int NPX = TH * TW;
  static constexpr int IH = TH + 2;
  static constexpr int IW = TW + 2;
  static constexpr int ROWB = IW * 64;          // bytes of one halo row
  static constexpr int HBUF = IH * ROWB;
  static constexpr int TAPB = 64 * 64;          // one tap of one 64-row group: 4 KB
  static constexpr int SLAB64 = 3 * TAPB;       // one kernel row of one 64-row group: 12 KB
  static constexpr int SLOT = WCO * SLAB64;
  static constexpr int NSLOT = 3;
  static constexpr int NWI = SLOT / 1024 / NW;  // DMA wave-instructions per wave per phase
  static constexpr int H_PIECES = IH * IW * 4;
  static constexpr int NHP = (H_PIECES + NTHR - 1) / NTHR;
  static constexpr int RING_OFF = 0;
  static constexpr int HALO_OFF = NSLOT * SLOT;
  // statistics scratch = the start of ring slot 2 (tap 0 of the tile's last phase: consumed before that phase's
  // synchronisation, and the next DMA into the slot is only issued behind the next tile's first synchronisation)
  static constexpr int RED_OFF = RING_OFF + 2 * SLOT;
  static constexpr int RED_BYTES = NW * 64 * 2 * 4;
  static constexpr int LDS_BYTES = HALO_OFF + 2 * HBUF;
  static_assert(NPX == WPX * NT * 16, "pixel tile must be covered by the pixel waves");
  static_assert(TW == 32 || TW == 16, "tile width");
  static_assert((SLOT / 1024) % NW == 0, "every wave issues the same number of DMA instructions");
  static_assert(RED_BYTES <= TAPB, "statistics scratch must stay inside tap 0 of the slot");
  static_assert(NTHR % 4 == 0, "a thread keeps its 16-byte slot of the 64-byte chunk");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

// Epilogue forms, chosen once per launch from the block-uniform flags (ring16_epilogue_form): inside a form the
// per-pixel loops test nothing but the lane's own bounds.
enum : int {
  RING16_EPI_GENERAL = 0,  // bias and / or ReLU, with or without residual and statistics (flags read once per tile)
  RING16_EPI_STATS = 1,    // statistics only: the forward convolution in front of a training-mode BatchNorm
  RING16_EPI_PLAIN = 2,    // nothing: dgrad
  RING16_EPI_RES = 3,      // residual only: dgrad joining a skip gradient
};

template <int WCO, int WPX, int NT, int TH, int TW, int OCC, bool PRO, int EPI>
__global__ void __launch_bounds__(64 * WCO * WPX, OCC) conv3x3_ring16_kernel(Ring3Args a) {
  using G = Ring16Geom<WCO, WPX, NT, TH, TW>;
  using T = ffa_bf16;
  constexpr int MT = G::MT;
  __shared__ __align__(16) unsigned char smem[G::LDS_BYTES];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wco = wave / WPX;
  const int wpx = wave % WPX;
  const int col = lane & 15;  // operand row (weights) / column (pixels) of a fragment; accumulator column
  const int kg = lane >> 4;   // channels 8*kg .. 8*kg+7 of a chunk; accumulator rows 4*kg .. 4*kg+3
  const int NC = a.nchunks;
  const int total_vb = ((a.npt + 7) / 8) * 8 * a.ncb;

  // ---- per-lane LDS read addresses (ring slot, tap, tile and kernel row are immediates) ----
  const int a0 = G::RING_OFF + wco * G::SLAB64 + col * 64 + ((kg ^ (((col >> 2) & 1) << 1)) * 16);
  int bB[NT][3];  // includes the base of the CURRENT halo buffer
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int n = wpx * (NT * 16) + nt * 16 + col;
    const int py = n / TW, px = n % TW;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const int hx = px + s;
      bB[nt][s] = G::HALO_OFF + (py * G::IW + hx) * 64 + ((kg ^ (((hx >> 2) & 1) << 1)) * 16);
    }
  }

  // ---- halo staging geometry (tile independent part) ----
  // Halo piece tid + k * NTHR = pixel q = (tid >> 2) + k * NTHR / 4 of the halo tile, 16-byte slot tid & 3.  The halo is
  // filled by LDS-DMA: the destination of a wave instruction is linear (base + lane * 16), so the thread owns PHYSICAL
  // slot tid & 3 of its pixel and fetches the logical slot that belongs there (the XOR goes on the source address).
  const int jj = tid & 3;

  struct TileId {
    int pt, cb, b, oy0, ox0;
  };
  // tile walk on the scalar unit: vb is block uniform, the divisions by ncb / tiles_x / tiles_y are multiplications by
  // the host's multipliers (a run-time division expands into a reciprocal sequence on the vector unit, per tile)
  auto tile_of = [&](int vb, int& cb) {
    unsigned r;
    const unsigned q = ffa_udiv_magic((unsigned)vb >> 3, (unsigned)a.ncb, a.m_ncb, r);
    cb = (int)r;
    return (int)(q * 8 + (vb & 7));  // the co blocks of a pixel tile share an XCD's L2 (speed only)
  };
  auto decode = [&](int vb) {
    TileId t;
    t.pt = __builtin_amdgcn_readfirstlane(tile_of(vb, t.cb));
    t.cb = __builtin_amdgcn_readfirstlane(t.cb);
    unsigned tx, ty;
    const unsigned t2 = ffa_udiv_magic((unsigned)t.pt, (unsigned)a.tiles_x, a.m_tx, tx);
    t.b = __builtin_amdgcn_readfirstlane((int)ffa_udiv_magic(t2, (unsigned)a.tiles_y, a.m_ty, ty));
    t.oy0 = __builtin_amdgcn_readfirstlane((int)ty * TH);
    t.ox0 = __builtin_amdgcn_readfirstlane((int)tx * TW);
    return t;
  };
  auto next_valid = [&](int vb) {
    int cb;
    while (vb < total_vb && tile_of(vb, cb) >= a.npt) vb += gridDim.x;
    return __builtin_amdgcn_readfirstlane(vb);
  };
  const int pix_bytes = a.Ci * 2;
  // the lane's halo pieces are launch constants: position in the halo tile and byte offset from the tile's halo origin
  // (input pixel (oy0 - 1, ox0 - 1), chunk 0) with the slot XOR applied -- a tile adds a scalar base and tests bounds
  int hyx[G::NHP];   // (hy << 16) | hx, negative past the last piece
  int hrel[G::NHP];
#pragma unroll
  for (int k = 0; k < G::NHP; ++k) {
    const int q = (tid >> 2) + k * (G::NTHR / 4);
    const int hy = q / G::IW, hx = q % G::IW;
    const int slot = jj ^ (((hx >> 2) & 1) << 1);
    hyx[k] = q < G::IH * G::IW ? ((hy << 16) | hx) : -1;
    hrel[k] = (hy * a.W + hx) * pix_bytes + slot * 16;
  }
  int hoff[G::NHP];  // byte offset of the piece from the input base (chunk 0), -1 = zero fill
  auto halo_offsets = [&](const TileId& t) {
    const int base = ((t.b * a.H + t.oy0 - 1) * a.W + t.ox0 - 1) * pix_bytes;
    const int ylo = 1 - t.oy0, yhi = a.H + 1 - t.oy0, xlo = 1 - t.ox0, xhi = a.W + 1 - t.ox0;
#pragma unroll
    for (int k = 0; k < G::NHP; ++k) {
      const int hy = hyx[k] >> 16, hx = hyx[k] & 0xffff;
      const bool ok = hyx[k] >= 0 && hy >= ylo && hy < yhi && hx >= xlo && hx < xhi;
      hoff[k] = ok ? base + hrel[k] : -1;
    }
  };

  const unsigned char* in_b = static_cast<const unsigned char*>(a.in);
  const unsigned char* w_all = static_cast<const unsigned char*>(a.w);

  // Weight DMA of one phase: the slab at `slab` (w_slab: kernel row `ph` of chunk ph / 3 of co block cb) -> ring slot
  // `slot`.  The source is a wave-uniform 64-bit base in scalar registers plus the lane's 16-byte offset: the main loop
  // advances the base by SLAB64 per phase and re-seats it where the tile or the co block changes, so no address is
  // rebuilt from (cb, ph) per instruction.
  const unsigned lane16 = lane * 16;
  auto w_slab = [&](int cb, int ph) {
    return w_all + (long long)(cb * WCO) * a.cb64_stride + (long long)ph * G::SLAB64;
  };
  auto issue_w = [&](const unsigned char* slab, int slot) {
#pragma unroll
    for (int i = 0; i < G::NWI; ++i) {
      const int ii = wave + i * G::NW;  // 1-KB piece of the slot (wave uniform)
      const unsigned char* src;
      if constexpr (WCO == 1) {
        src = slab + ii * 1024;
      } else {
        const int g64 = ii / (G::SLAB64 / 1024), pi = ii % (G::SLAB64 / 1024);
        src = slab + (long long)g64 * a.cb64_stride + pi * 1024;
      }
      ffa_lds_dma16_uniform(src, lane16, (unsigned)(size_t)(__attribute__((address_space(3))) void*)(
                                             smem + G::RING_OFF + slot * G::SLOT + ii * 1024));
    }
  };
  // LDS-DMA halo fill (no prologue): chunk `chunk` of the tile hoff[] describes -> halo buffer `buf`.  The tail
  // instruction runs with the lanes past the last piece masked off (they would write into the other buffer).
  auto dma_h = [&](int chunk, int buf) {
    const unsigned char* base = in_b + chunk * 64;
    const unsigned char* zero = reinterpret_cast<const unsigned char*>(ffa_zero16);
#pragma unroll
    for (int k = 0; k < G::NHP; ++k) {
      const unsigned char* src = hoff[k] >= 0 ? base + (unsigned)hoff[k] : zero;
      const unsigned dst = (unsigned)(size_t)(__attribute__((address_space(3))) void*)(
          smem + G::HALO_OFF + buf * G::HBUF + (wave * 64 + k * G::NTHR) * 16);
      if (k + 1 < G::NHP || G::H_PIECES % G::NTHR == 0) {
        ffa_lds_dma16(src, dst);
      } else if (wave * 64 + k * G::NTHR < G::H_PIECES) {  // wave uniform
        if (tid + k * G::NTHR < G::H_PIECES) ffa_lds_dma16(src, dst);
      }
    }
  };
  // PRO ("normalise on load"): the convolution reads relu(in * pro_sc[c] + pro_sh[c]).  The raw halo arrives by DMA;
  // once this wave's own pieces have landed (its vmcnt wait) thread t rewrites, in LDS, the pieces of LOGICAL slot
  // t & 3 of its pixels -- the same 8 channels for every piece (one scale / shift load per chunk), and pieces that this
  // very wave's DMA wrote (pixel q is filled by lanes 4*(q % 64) .. +3) -- skipping the zero padding (hoff < 0: the
  // padding of the normalised tensor is zero, not relu(shift)).  Same fma / max / rounding as ffa_bn_apply.
  auto fix_h = [&](int chunk, int buf) {
    if constexpr (PRO) {
      float psc[8], psh[8];
      const int c0 = chunk * 32 + jj * 8;
      ffa_load8<float>(a.pro_sc + c0, psc);
      ffa_load8<float>(a.pro_sh + c0, psh);
      unsigned char* base = smem + G::HALO_OFF + buf * G::HBUF;
#pragma unroll
      for (int k = 0; k < G::NHP; ++k) {
        const int q = (tid >> 2) + k * (G::NTHR / 4);
        const int hx = q % G::IW;
        if ((k + 1 < G::NHP || G::H_PIECES % G::NTHR == 0 || q < G::IH * G::IW) && hoff[k] >= 0) {
          ffa_u32x4* ptr = reinterpret_cast<ffa_u32x4*>(base + q * 64 + ((jj ^ (((hx >> 2) & 1) << 1)) * 16));
          ffa_u32x4 v = *ptr;
          float f[8];
          f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
          f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
          f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
          f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
#pragma unroll
          for (int e = 0; e < 8; ++e) f[e] = fmaxf(__builtin_fmaf(f[e], psc[e], psh[e]), 0.f);
          v.x = ffa_pack_bf16x2(f[0], f[1]);
          v.y = ffa_pack_bf16x2(f[2], f[3]);
          v.z = ffa_pack_bf16x2(f[4], f[5]);
          v.w = ffa_pack_bf16x2(f[6], f[7]);
          *ptr = v;
        }
      }
    }
  };

  int vb = next_valid(blockIdx.x);
  if (vb >= total_vb) return;
  TileId cur = decode(vb);

  // ---- prologue of the block's first tile (the only exposed one) ----
  halo_offsets(cur);
  dma_h(0, 0);
  issue_w(w_slab(cur.cb, 0), 0);
  issue_w(w_slab(cur.cb, 1), 1);
  const unsigned char* wp = w_slab(cur.cb, 2);  // the slab the next phase synchronisation issues
  if constexpr (PRO) {
    ffa_wait_vm<0>();
    fix_h(0, 0);
  }
  ffa_wait_vm_lgkm_barrier<0>();  // slabs 0 and 1 and halo chunk 0 are in LDS (and normalised)
  int hb = 0;
  int hd = G::HBUF;  // byte distance from the current halo buffer to the other one

  ffa_u32x4 fa[3][MT], fb[3][NT];  // fragment sets by step of the phase (two of them live at a time)
  int bBn[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) bBn[nt] = bB[nt][0] + hd;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) fa[0][mt] = *reinterpret_cast<const ffa_u32x4*>(smem + a0 + mt * 1024);
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) fb[0][nt] = *reinterpret_cast<const ffa_u32x4*>(smem + bB[nt][0]);

  ffa_f32x4 acc[MT][NT];

  while (true) {
    const int nvb = next_valid(vb + gridDim.x);
    const bool has_next = nvb < total_vb;
    const TileId nxt = decode(has_next ? nvb : vb);
    const unsigned char* wnext = w_slab(nxt.cb, 0);

#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        acc[mt][nt] = ffa_f32x4{0.f, 0.f, 0.f, 0.f};
        asm volatile("" : "+v"(acc[mt][nt]));  // zeroed here, once: not again on every path into the chunk loop
      }

    for (int c = 0; c < NC; ++c) {
      const bool last_c = (c + 1 == NC);
      const bool hvalid = !last_c || has_next;
      if (last_c && has_next) halo_offsets(nxt);
      const int hchunk = last_c ? 0 : c + 1;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const unsigned char* sA = smem + a0 + r * G::SLOT;
        const unsigned char* sAn = smem + a0 + ((r + 1) % 3) * G::SLOT;
#pragma unroll
        for (int st = 0; st < 3; ++st) {
          __builtin_amdgcn_sched_barrier(0);
          // ---- request the fragments of the next step ----
          if (st < 2) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
              fa[st + 1][mt] = *reinterpret_cast<const ffa_u32x4*>(sA + (st + 1) * G::TAPB + mt * 1024);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
              fb[st + 1][nt] = *reinterpret_cast<const ffa_u32x4*>(smem + bB[nt][st + 1] + r * G::ROWB);
          } else {  // step 0 of the next phase: ring slot r + 1, halo row r + 1 (or row 0 of the next chunk)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) fa[0][mt] = *reinterpret_cast<const ffa_u32x4*>(sAn + mt * 1024);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
              if (r < 2) fb[0][nt] = *reinterpret_cast<const ffa_u32x4*>(smem + bB[nt][0] + (r + 1) * G::ROWB);
              else fb[0][nt] = *reinterpret_cast<const ffa_u32x4*>(smem + bBn[nt]);
            }
          }
          // ---- multiply step st ----
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(ffa_bf16x8, fa[st][mt]),
                                                                    __builtin_bit_cast(ffa_bf16x8, fb[st][nt]),
                                                                    acc[mt][nt], 0, 0, 0);
#pragma unroll
          for (int i = 0; i < MT * NT; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            if (i < MT + NT) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          }
          if (st == 0) {
            __builtin_amdgcn_sched_barrier(0);
            // next chunk's halo into the other buffer (requested a whole chunk ago), then the phase meets: every
            // wave's DMA of the next phase has landed (issued a phase ago) and every wave is done with the previous
            // phase's ring slot -> refill it
            // vector-memory queue, oldest first -- at r = 0: W(p+1); at r = 1: W(p+1), then the NHP halo pieces issued
            // behind it (they may stay in flight for another phase); at r = 2: halo pieces, W(p+1): the halo is read
            // from step 2 of this phase on, so everything must have landed
            if (r == 1 && hvalid) {  // (no halo fill behind W(p+1) when this is the block's last chunk: plain wait)
              // exact count per wave: the tail instruction of the halo fill exists only in the waves that own pieces
              // of it (a wave that waited for one operation too few would publish a weight slab still in flight)
              constexpr bool TAIL = G::H_PIECES % G::NTHR != 0;
              if (!TAIL || wave * 64 + (G::NHP - 1) * G::NTHR < G::H_PIECES) ffa_wait_vm_barrier<G::NHP>();
              else ffa_wait_vm_barrier<G::NHP - 1>();
            } else if (PRO && r == 2) {
              ffa_wait_vm<0>();
              // the tile whose halo this is: hoff[] already describes it (the next chunk of `cur`, or chunk 0 of `nxt`)
              if (hvalid) fix_h(hchunk, hb ^ 1);
              ffa_wait_vm_lgkm_barrier<0>();  // the rewritten pieces must be in LDS before the block meets
            } else {
              ffa_wait_vm_barrier<0>();
            }
            // weight slab two phases ahead: this tile's, the next tile's first ones, or (no next tile) a re-read of
            // this tile's last slab, which lands in a slot nobody reads again (keeps every wave's DMA count uniform)
            issue_w(wp, (r + 2) % 3);
            if (last_c && r == 0) {
              if (has_next) wp = wnext;
            } else if (hvalid) {
              wp += G::SLAB64;
            }
            if (r == 0 && hvalid) dma_h(hchunk, hb ^ 1);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      // the next chunk reads the other halo buffer
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int s = 0; s < 3; ++s) bB[nt][s] += hd;
      }
      hb ^= 1;
      hd = -hd;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) bBn[nt] = bB[nt][0] + hd;
    }

    // ---- epilogue of `cur`: lane (col, kg) owns pixel n = wave px base + nt*16 + col and 16 consecutive channels ----
    // Straight line per form: every load of the tile (residual vectors, bias) is requested first and waited for
    // once, the eight output vectors are finished in registers, then stored back to back -- no wait between two
    // stores -- and the statistics are taken from the stored words afterwards.  A lane reads its own residual
    // elements before it writes them, so res == out stays legal.
    {
      T* out = static_cast<T*>(a.out);
      const T* res = static_cast<const T*>(a.res);
      constexpr bool GEN = EPI == RING16_EPI_GENERAL;
      const bool has_bias = GEN && a.bias != nullptr;
      const bool has_res = EPI == RING16_EPI_RES || (GEN && res != nullptr);
      const bool do_relu = GEN && a.relu != 0;
      const bool want_stats = EPI == RING16_EPI_STATS || (GEN && a.stats != nullptr);
      const int co_lane = cur.cb * G::BCO + wco * 64 + 16 * kg;
      const bool cok[2] = {co_lane < a.Co, co_lane + 8 < a.Co};
      long long pix[NT];  // element offset of the lane's pixel
      bool ok[NT];        // ... which lies inside the image
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n = wpx * (NT * 16) + nt * 16 + col;
        const int oy = cur.oy0 + n / TW, ox = cur.ox0 + n % TW;
        ok[nt] = oy < a.H && ox < a.W;
        pix[nt] = ((long long)(cur.b * a.H + oy) * a.W + ox) * (long long)a.Co;
      }
      // -0.0 is the neutral element of the f32 addition for EVERY value (x + -0.0 == x bit for bit, +0.0 included):
      // the general form adds it where a launch has no bias / no residual instead of branching per vector
      constexpr unsigned NEG0X2 = 0x80008000u;
      ffa_u32x4 rw[NT][2];
      float bv[GEN ? 16 : 1];
      if constexpr (GEN || EPI == RING16_EPI_RES) {
        if (has_res) {
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int h = 0; h < 2; ++h)  // a lane outside the image / past Co reads the tensor's first vector and drops it
              rw[nt][h] = *reinterpret_cast<const ffa_u32x4*>((ok[nt] && cok[h]) ? res + pix[nt] + co_lane + 8 * h : res);
        } else {
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int h = 0; h < 2; ++h) rw[nt][h] = ffa_u32x4{NEG0X2, NEG0X2, NEG0X2, NEG0X2};
        }
      }
      if constexpr (GEN) {
        if (has_bias) {  // the lane's 16 bias values: once per tile, in flight together with the residual
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            float b8[8];
            ffa_load8<float>(cok[h] ? a.bias + co_lane + 8 * h : a.bias, b8);
#pragma unroll
            for (int i = 0; i < 8; ++i) bv[8 * h + i] = b8[i];
          }
        } else {
#pragma unroll
          for (int i = 0; i < 16; ++i) bv[i] = -0.f;
        }
      }
      if constexpr (GEN || EPI == RING16_EPI_RES) ffa_wait_vm<0>();  // the one wait of the tile's loads
      ffa_u32x4 u[NT][2];  // the stored words: rounded once, also what the statistics are taken from
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          float v[8];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            v[i] = acc[2 * h][nt][i];
            v[4 + i] = acc[2 * h + 1][nt][i];
          }
          if constexpr (GEN) {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] += bv[8 * h + i];
          }
          if constexpr (GEN || EPI == RING16_EPI_RES) {
            const ffa_u32x4 r4 = rw[nt][h];
            const float rv[8] = {__uint_as_float(r4.x << 16), __uint_as_float(r4.x & 0xffff0000u),
                                 __uint_as_float(r4.y << 16), __uint_as_float(r4.y & 0xffff0000u),
                                 __uint_as_float(r4.z << 16), __uint_as_float(r4.z & 0xffff0000u),
                                 __uint_as_float(r4.w << 16), __uint_as_float(r4.w & 0xffff0000u)};
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] += rv[i];
          }
          if constexpr (GEN) {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = do_relu ? fmaxf(v[i], 0.f) : v[i];
          }
          u[nt][h].x = ffa_pack_bf16x2(v[0], v[1]);
          u[nt][h].y = ffa_pack_bf16x2(v[2], v[3]);
          u[nt][h].z = ffa_pack_bf16x2(v[4], v[5]);
          u[nt][h].w = ffa_pack_bf16x2(v[6], v[7]);
          // pinned here: left alone the compiler sinks this arithmetic into the (per-lane conditional) store blocks
          // below, and its own wait for the residual load in front of it then also waits for the stores before it
          asm volatile("" : "+v"(u[nt][h]));
        }
      }
      __builtin_amdgcn_sched_barrier(0);  // every vector is finished before the first store
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int h = 0; h < 2; ++h)
          if (ok[nt] && cok[h]) *reinterpret_cast<ffa_u32x4*>(out + pix[nt] + co_lane + 8 * h) = u[nt][h];
      if (want_stats) {
        float st[32];  // [16 sums | 16 sums of squares] of this lane's channels, taken from the stored words
#pragma unroll
        for (int i = 0; i < 32; ++i) st[i] = 0.f;
        // a vector the lane did not store counts as zeros: st starts at +0.0 and a sum that started there is never
        // -0.0, so adding +0.0 (and 0 * 0) leaves every bit of it -- no per-lane branch around the chains
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const bool stored = ok[nt] && cok[h];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
              const unsigned word = stored ? u[nt][h][w] : 0u;
              const float rr[2] = {__uint_as_float(word << 16), __uint_as_float(word & 0xffff0000u)};
#pragma unroll
              for (int e = 0; e < 2; ++e) {
                const int ch = 8 * h + 2 * w + e;
                st[ch] += rr[e];
                st[16 + ch] = __builtin_fmaf(rr[e], rr[e], st[16 + ch]);  // explicit: all conv kernels round alike
              }
            }
          }
        }
        // transposing reduction over the 16 lanes that share kg: afterwards lane col holds entries 2*col and 2*col + 1
        // of [sums | sums of squares]
#pragma unroll
        for (int bit = 3; bit >= 0; --bit) {
          const int n = 32 >> (3 - bit);
          const bool up = (col >> bit) & 1;
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            if (j < n / 2) {
              float lo = st[j], hi = st[j + n / 2];
              asm volatile("" : "+v"(lo), "+v"(hi));
              const float keep = up ? hi : lo;
              const float send = up ? lo : hi;
              st[j] = keep + __shfl_xor(send, 1 << bit, 64);
            }
          }
        }
        float* red = reinterpret_cast<float*>(smem + G::RED_OFF);
        red[(wave * 64 + lane) * 2 + 0] = st[0];
        red[(wave * 64 + lane) * 2 + 1] = st[1];
        ffa_wait_lgkm_barrier();
        if (tid < 128 * WCO) {
          const int wc = tid >> 7, t7 = tid & 127;
          const int j = t7 & 1;
          const int ln = t7 >> 1;
          float t = 0.f;
#pragma unroll
          for (int w = 0; w < WPX; ++w) t += red[((wc * WPX + w) * 64 + ln) * 2 + j];
          const int cl = ln & 15, kq = ln >> 4;
          const int which = cl >> 3;
          const int ch = cur.cb * G::BCO + wc * 64 + 16 * kq + (cl & 7) * 2 + j;
          if (ch < a.Co) a.stats[((size_t)cur.pt * 2 + which) * a.Co + ch] = t;
        }
        ffa_wait_lgkm_barrier();  // red is reused by the next tile
      }
    }
    if (!has_next) break;
    vb = nvb;
    cur = nxt;
  }
  // the trailing DMA (re-reads of the last slab) must not outlive the block's LDS allocation
  ffa_wait_vm<0>();
}

// ------------------------------------------------------------------------------------------------
// host side

// The epilogue form of a launch: the three forms of the training step, anything with a bias or a ReLU is general.
static int ring16_epilogue_form(const Ring3Args& a) {
  if (a.bias || a.relu) return RING16_EPI_GENERAL;
  if (a.stats) return a.res ? RING16_EPI_GENERAL : RING16_EPI_STATS;
  return a.res ? RING16_EPI_RES : RING16_EPI_PLAIN;
}

template <int WCO, int WPX, int NT, int TH, int TW, int OCC, int EPI>
static void ring16_launch_form(const Ring3Args& a, int grid, hipStream_t stream) {
  if (!a.pro_sc)  // measurement session open (bench.py): the kernel's own duration from launch-attached events
    ffa_launch_timed(WCO == 2 ? FFA_KT_RING16_128CO : (TW == 32 ? FFA_KT_RING16_8x32 : FFA_KT_RING16_16x16),
                     conv3x3_ring16_kernel<WCO, WPX, NT, TH, TW, OCC, false, EPI>, dim3(grid), dim3(64 * WCO * WPX),
                     stream, a);
  else
    hipLaunchKernelGGL((conv3x3_ring16_kernel<WCO, WPX, NT, TH, TW, OCC, true, EPI>), dim3(grid),
                       dim3(64 * WCO * WPX), 0, stream, a);
}

template <int WCO, int WPX, int NT, int TH, int TW, int OCC>
static int ring16_launch(const Ring3Args& a, int grid, hipStream_t stream) {
  switch (ring16_epilogue_form(a)) {
    case RING16_EPI_STATS: ring16_launch_form<WCO, WPX, NT, TH, TW, OCC, RING16_EPI_STATS>(a, grid, stream); break;
    case RING16_EPI_PLAIN: ring16_launch_form<WCO, WPX, NT, TH, TW, OCC, RING16_EPI_PLAIN>(a, grid, stream); break;
    case RING16_EPI_RES: ring16_launch_form<WCO, WPX, NT, TH, TW, OCC, RING16_EPI_RES>(a, grid, stream); break;
    default: ring16_launch_form<WCO, WPX, NT, TH, TW, OCC, RING16_EPI_GENERAL>(a, grid, stream); break;
  }
  return ffa_check_launch("conv3x3_ring16");
}

template <typename T, int WCO, int WPX, int NT, int TH, int TW, int OCC>
static int ring_launch(const Ring3Args& a, int grid, hipStream_t stream) {
  if (a.pro_sc)
    hipLaunchKernelGGL((conv3x3_ring_kernel<T, WCO, WPX, NT, TH, TW, OCC, true>), dim3(grid), dim3(64 * WCO * WPX), 0,
                       stream, a);
  else
    hipLaunchKernelGGL((conv3x3_ring_kernel<T, WCO, WPX, NT, TH, TW, OCC, false>), dim3(grid), dim3(64 * WCO * WPX), 0,
                       stream, a);
  return ffa_check_launch("conv3x3_ring");
}

// Ring layout: the plain form of a 3x3 stride-1 pad-1 convolution, with statistics and / or the prologue.
// Tile configuration (r->variant).  cfg 1: 64 co x 8x32 px, 4 waves, two blocks per CU; cfg 2: 64 co x 16x16 px,
// 4 waves; cfg 4: 128 co x 8x32 px, 8 waves.  (cfg 3 / 5 of round 2 -- 64 co x 128 px per wave -- measured slower and
// are gone; their numbers map to 4 / 1.)
int ffa_ring_route(const ffa_conv_call_t& c, ffa_conv_route_t* r) {
  FFA_REQUIRE(c.kh == 3 && c.kw == 3 && c.stride == 1 && c.pad == 1 && c.dil == 1 && c.Hi == c.Ho && c.Wi == c.Wo &&
                  c.bnx == nullptr,
              "conv: a ring-layout operand serves plain 3x3 stride-1 pad-1 convolutions only");
  FFA_REQUIRE((c.Ci * ffa_conv_elem_bytes(c.dtype)) % 64 == 0 && c.co_rows > 0 && c.co_rows % 64 == 0,
              "ring conv: bad dims (Ci %d, Co %d, rows %d)", c.Ci, c.Co, c.co_rows);
  const int W = c.Wo;
  const char* force = getenv("FFA_RING_CFG");
  int cfg = force ? atoi(force) : -1;
  if (cfg < 0) cfg = (W < 32) ? 2 : 1;
  if (cfg == 3) cfg = 4;
  if (cfg == 5) cfg = 1;
  if (cfg == 4 && (c.co_rows % 128 != 0 || W < 32)) cfg = (W < 32) ? 2 : 1;
  if (cfg == 1 && W < 32) cfg = 2;
  int bco = 64;
  switch (cfg) {
    case 1: r->th = 8; r->tw = 32; break;
    case 2: r->th = 16; r->tw = 16; break;
    case 4: r->th = 8; r->tw = 32; bco = 128; break;
    default:
      ffa_set_error("ring conv: no configuration for %dx%d, %d rows", c.Ho, c.Wo, c.co_rows);
      return FFA_ERR_UNSUPPORTED;
  }
  r->variant = cfg;
  r->kernel = (c.dtype == FFA_BF16) ? FFA_CONV_KERNEL_RING16 : FFA_CONV_KERNEL_RING;
  r->tiles_x = ffa_cdiv(W, r->tw);
  r->tiles_y = ffa_cdiv(c.Ho, r->th);
  r->ntiles = c.B * r->tiles_x * r->tiles_y;
  r->ncb = c.co_rows / bco;
  const int total = ffa_cdiv(r->ntiles, 8) * 8 * r->ncb;
  const char* pg = getenv("FFA_RING_GRID");
  // two 4-wave blocks per CU (cfg 1; cfg 2 on the bf16 kernel), one 8-wave block (cfg 4)
  int cap = pg ? atoi(pg) : ((cfg == 1 || (cfg == 2 && c.dtype == FFA_BF16)) ? 512 : 256);
  cap = cap < 8 ? 8 : (cap / 8) * 8;
  r->grid = total < cap ? total : cap;
  return 0;
}

int ffa_ring_launch(const ffa_conv_call_t& c, const ffa_conv_route_t& r, hipStream_t stream) {
  Ring3Args a;
  a.in = c.in;
  a.w = c.w;
  a.out = c.out;
  a.bias = c.bias;
  a.stats = c.stats;
  a.res = c.residual;
  a.pro_sc = c.pro_scale;
  a.pro_sh = c.pro_shift;
  a.B = c.B; a.H = c.Ho; a.W = c.Wo; a.Ci = c.Ci; a.Co = c.Co;
  a.relu = c.relu;
  a.nchunks = c.Ci * ffa_conv_elem_bytes(c.dtype) / 64;
  a.tiles_x = r.tiles_x;
  a.tiles_y = r.tiles_y;
  a.npt = r.ntiles;
  a.ncb = r.ncb;
  a.cb64_stride = (long long)a.nchunks * 3 * (3 * 2 * 64 * 32);
  a.m_ncb = ffa_udiv_magic_of(a.ncb);
  a.m_tx = ffa_udiv_magic_of(a.tiles_x);
  a.m_ty = ffa_udiv_magic_of(a.tiles_y);
  if (c.dtype == FFA_BF16) {  // v_mfma_f32_16x16x32_bf16 kernel (NT counts 16-pixel fragments there)
    switch (r.variant) {
      case 1: return ring16_launch<1, 4, 4, 8, 32, 2>(a, r.grid, stream);
      case 2: return ring16_launch<1, 4, 4, 16, 16, 2>(a, r.grid, stream);
      case 4: return ring16_launch<2, 4, 4, 8, 32, 2>(a, r.grid, stream);
    }
    return FFA_ERR_UNSUPPORTED;
  }
  switch (r.variant) {
    case 1: return ring_launch<float, 1, 4, 2, 8, 32, 2>(a, r.grid, stream);
    case 2: return ring_launch<float, 1, 4, 2, 16, 16, 1>(a, r.grid, stream);
    case 4: return ring_launch<float, 2, 4, 2, 8, 32, 2>(a, r.grid, stream);
  }
  return FFA_ERR_UNSUPPORTED;
}

#if FFA_RING_TRACE
extern "C" int ffa_ring_trace_read(long long* host_dst, int n) {
  if (n > 1024 * 8) n = 1024 * 8;
  (void)hipDeviceSynchronize();
  return (int)hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(ffa_ring_trace_buf), (size_t)n * sizeof(long long));
}
#endif
