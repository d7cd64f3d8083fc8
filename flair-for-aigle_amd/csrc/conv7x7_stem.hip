// The ResNet stem: 7x7 stride-2 pad-3 convolution of a 5-channel tile into 64 channels (bf16; round 3).
//
// Replaces the generic conv_igemm_kernel<7, 7, 2> for torchvision's `conv1 = Conv2d(in, 64, 7, 2, 3, bias=False)` as smp's
// ResNetEncoder keeps it (reference: flair_hub/models/monotemp_model.py:68-92 -> smp.create_model; oracle/unet_resnet34.py).
// The generic kernel multiplies one 16-channel pixel (the NHWC pitch of the 5-channel input) per 32-byte k-step: K = 49
// taps x 16 = 784, of which 245 are real -- it ran at 0.18 PFLOP/s of useful work, 3.4x its HBM floor.  Here:
//   * only the first 8 channels (16 bytes) of every input pixel are staged (LDS-DMA, per-lane source address: the DMA
//     gathers one 16-byte piece per pixel; pad channels 5..7 hold zeros by the layout contract);
//   * one K = 32 step of v_mfma_f32_16x16x32_bf16 = FOUR horizontally adjacent taps x 8 channels: lane (pixel, kg) reads
//     the 16 bytes of input pixel 2 * ox + 4 * half + kg -- K = 7 rows x 2 halves x 32 = 448 (the eighth tap has zero
//     weights), 43 % fewer matrix instructions;
//   * even and odd input columns live in separate LDS planes, so the 16 lanes of a fragment (stride-2 pixels) read 256
//     consecutive bytes: conflict-free ds_read_b128;
//   * the whole weight operand (14 k-steps x 64 rows x 64 B = 56 KB, ring16's row permutation and slot swizzle) stays in
//     LDS for the launch; persistent blocks of eight waves walk 16 x 32-pixel output tiles, the halo of the next tile
//     arrives while the current one is multiplied;
//   * epilogue as conv3x3_ring16_kernel's: a lane owns 16 consecutive channels of its pixel, optional bias / ReLU,
//     BatchNorm batch statistics of the stored values (per-tile partial rows for ffa_bn_finalize).
#include "ffa_gfx950.h"

#include "conv7x7_stem.h"
#include "conv_call.h"

struct StemArgs {
  const void* in;   // [B][Hi][Wi][16] bf16
  const void* w;    // stem layout of conv_pack.hip
  void* out;        // [B][Ho][Wo][Co] bf16
  const float* bias;
  float* stats;     // [npt][2][Co] or null
  int B, Hi, Wi, Ho, Wo, Co;
  int relu;
  int tiles_x, tiles_y, npt;
};

__global__ void __launch_bounds__(512) conv7x7_stem_kernel(StemArgs a) {
  using G = StemGeom;
  __shared__ __align__(16) unsigned char smem[G::LDS_BYTES];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, kg = lane >> 4;

  // ---- weights: once per block ----
  {
    const unsigned char* wsrc = static_cast<const unsigned char*>(a.w);
#pragma unroll
    for (int k = 0; k < G::WP / G::NTHR; ++k) {
      const int p = tid + k * G::NTHR;
      ffa_lds_dma16(wsrc + (size_t)p * 16,
                 (unsigned)(size_t)(__attribute__((address_space(3))) void*)(smem + G::W_OFF + (wave * 64 + k * G::NTHR) * 16));
    }
  }

  // ---- halo pieces of this thread, fixed for the launch: piece p = (row hy, parity, pair xi) <- input pixel
  //      (2 * oy0 - 3 + hy, 2 * ox0 - 3 + 2 * xi + parity); source offset from the tile's origin pixel in bytes ----
  int pinfo[G::NHW];  // hy << 8 | hx, -1: no piece
  int poff[G::NHW];
#pragma unroll
  for (int k = 0; k < G::NHW; ++k) {
    const int p = tid + k * G::NTHR;
    const int hy = p / G::ROWP, rem = p % G::ROWP;
    const int hx = 2 * (rem % G::IWH) + rem / G::IWH;
    pinfo[k] = (p < G::HP && hx < 2 * G::TW + 5) ? ((hy << 8) | hx) : -1;
    poff[k] = (hy * a.Wi + hx) * 32;
  }
  const unsigned char* in_b = static_cast<const unsigned char*>(a.in);
  const unsigned char* zero = reinterpret_cast<const unsigned char*>(ffa_zero16);

  auto tile_origin = [&](int t, int& b, int& oy0, int& ox0) {
    const int tx = t % a.tiles_x;
    const int t2 = t / a.tiles_x;
    oy0 = (t2 % a.tiles_y) * G::TH;
    b = t2 / a.tiles_y;
    ox0 = tx * G::TW;
  };
  auto issue_halo = [&](int t, int buf) {
    int b, oy0, ox0;
    tile_origin(t, b, oy0, ox0);
    const int iy0 = 2 * oy0 - 3, ix0 = 2 * ox0 - 3;
    const unsigned char* base = in_b + ((long long)(b * a.Hi + iy0) * a.Wi + ix0) * 32;  // may lie outside: only valid pieces use it
#pragma unroll
    for (int k = 0; k < G::NHW; ++k) {
      const int info = pinfo[k];
      const int iy = iy0 + (info >> 8), ix = ix0 + (info & 255);
      const bool valid = info >= 0 && (unsigned)iy < (unsigned)a.Hi && (unsigned)ix < (unsigned)a.Wi;
      const unsigned char* src = valid ? base + poff[k] : zero;
      const unsigned dst = (unsigned)(size_t)(__attribute__((address_space(3))) void*)(
          smem + G::H_OFF + buf * G::HBYTES + (wave * 64 + k * G::NTHR) * 16);
      if (k + 1 < G::NHW || G::HP % G::NTHR == 0) {
        ffa_lds_dma16(src, dst);
      } else if (wave * 64 + k * G::NTHR < G::HP) {      // wave uniform
        if (tid + k * G::NTHR < G::HP) ffa_lds_dma16(src, dst);  // (lanes past the last piece would write into the next buffer)
      }
    }
  };

  // ---- fragment addressing ----
  // A: k-step image [64 rows][64 B]; lane (row = col, kg) reads slot kg of row mt * 16 + col, slot ^= 2 when bit 2 of the row
  const int a0 = G::W_OFF + col * 64 + ((kg ^ (((col >> 2) & 1) << 1)) * 16);
  // B: fragment nt = output row 2 * wave + (nt >> 1), columns (nt & 1) * 16 + col; tap 4 * half + kg of kernel row r reads
  // input column 2 * ocol + 4 * half + kg: parity kg & 1, pair index ocol + 2 * half + (kg >> 1)
  int b0[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int py = 2 * wave + (nt >> 1), ocol = (nt & 1) * 16 + col;
    b0[nt] = G::H_OFF + (((2 * py) * 2 + (kg & 1)) * G::IWH + ocol + (kg >> 1)) * 16;
  }

  ffa_f32x4 acc[4][4];
  int t = blockIdx.x;
  if (t < a.npt) issue_halo(t, 0);
  int buf = 0;
  for (; t < a.npt; t += gridDim.x) {
    ffa_wait_vm_barrier<0>();  // this tile's halo (and the weights) landed; other buffer free
    const int tn = t + gridDim.x;
    if (tn < a.npt) issue_halo(tn, buf ^ 1);
    const unsigned char* sH = smem + buf * G::HBYTES;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = ffa_f32x4{0.f, 0.f, 0.f, 0.f};
    ffa_u32x4 fa[2][4], fb[2][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) fa[0][mt] = *reinterpret_cast<const ffa_u32x4*>(smem + a0 + mt * 1024);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) fb[0][nt] = *reinterpret_cast<const ffa_u32x4*>(sH + b0[nt]);
#pragma unroll
    for (int ks = 0; ks < G::KSTEPS; ++ks) {
      const int cur = ks & 1, nxt = cur ^ 1;
      if (ks + 1 < G::KSTEPS) {
        const int r = (ks + 1) >> 1, half = (ks + 1) & 1;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
          fa[nxt][mt] = *reinterpret_cast<const ffa_u32x4*>(smem + a0 + (ks + 1) * 4096 + mt * 1024);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          fb[nxt][nt] = *reinterpret_cast<const ffa_u32x4*>(sH + b0[nt] + (r * G::ROWP + 2 * half) * 16);
      }
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(ffa_bf16x8, fa[cur][mt]),
                                                                __builtin_bit_cast(ffa_bf16x8, fb[cur][nt]), acc[mt][nt],
                                                                0, 0, 0);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        if (i < 8 && ks + 1 < G::KSTEPS) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
    }

    // ---- epilogue: lane (col, kg) owns pixel (2 * wave + (nt >> 1), (nt & 1) * 16 + col) and channels 16 * kg .. + 15 ----
    {
      int b, oy0, ox0;
      tile_origin(t, b, oy0, ox0);
      ffa_bf16* out = static_cast<ffa_bf16*>(a.out);
      float st[32];
      const bool want_stats = a.stats != nullptr;
#pragma unroll
      for (int i = 0; i < 32; ++i) st[i] = 0.f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int oy = oy0 + 2 * wave + (nt >> 1), ox = ox0 + (nt & 1) * 16 + col;
        if (oy >= a.Ho || ox >= a.Wo) continue;
        const long long pix = ((long long)(b * a.Ho + oy) * a.Wo + ox) * (long long)a.Co;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int c0 = 16 * kg + 8 * h;
          float v[8];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            v[i] = acc[2 * h][nt][i];
            v[4 + i] = acc[2 * h + 1][nt][i];
          }
          if (a.bias) {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] += a.bias[c0 + i];
          }
          if (a.relu) {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = fmaxf(v[i], 0.f);
          }
          ffa_u32x4 u;
          u.x = ffa_pack_bf16x2(v[0], v[1]);
          u.y = ffa_pack_bf16x2(v[2], v[3]);
          u.z = ffa_pack_bf16x2(v[4], v[5]);
          u.w = ffa_pack_bf16x2(v[6], v[7]);
          *reinterpret_cast<ffa_u32x4*>(out + pix + c0) = u;
          if (want_stats) {
            const float rr[8] = {__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u),
                                 __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u),
                                 __uint_as_float(u.z << 16), __uint_as_float(u.z & 0xffff0000u),
                                 __uint_as_float(u.w << 16), __uint_as_float(u.w & 0xffff0000u)};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              st[h * 8 + i] += rr[i];
              st[16 + h * 8 + i] = __builtin_fmaf(rr[i], rr[i], st[16 + h * 8 + i]);
            }
          }
        }
      }
      if (want_stats) {
        // transposing reduction over the 16 lanes that share kg (conv3x3_ring16_kernel's): afterwards lane col holds
        // entries 2 * col and 2 * col + 1 of [16 sums | 16 sums of squares] of channels 16 * kg ..
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
        __syncthreads();
        if (tid < 128) {
          const int j = tid & 1, ln = tid >> 1;
          float s = 0.f;
#pragma unroll
          for (int w = 0; w < G::NW; ++w) s += red[(w * 64 + ln) * 2 + j];
          const int cl = ln & 15, kq = ln >> 4;
          const int which = cl >> 3;
          const int ch = 16 * kq + (cl & 7) * 2 + j;
          a.stats[((size_t)t * 2 + which) * a.Co + ch] = s;
        }
        // (red is written again only behind the next tile's barrier)
      }
    }
    buf ^= 1;
  }
  ffa_wait_vm<0>();  // nothing of this block may still be writing its LDS
}

bool ffa_stem_takes_layer(int dtype, int kh, int kw, int stride, int cout, int ci_pitch) {
  return dtype == FFA_BF16 && kh == 7 && kw == 7 && stride == 2 && cout == 64 && ci_pitch == 16;
}

// Stem layout: the plain form of the bf16 7x7 stride-2 pad-3 convolution, with statistics; no residual input.
int ffa_stem_route(const ffa_conv_call_t& c, ffa_conv_route_t* r) {
  FFA_REQUIRE(c.dtype == FFA_BF16 && c.kh == 7 && c.kw == 7 && c.stride == 2 && c.pad == 3 && c.dil == 1 &&
                  c.bnx == nullptr && c.residual == nullptr,
              "conv: a stem-layout operand serves the bf16 7x7 stride-2 pad-3 convolution only (no residual input)");
  FFA_REQUIRE(c.Ci == 16 && c.Co == 64, "stem conv: input pitch 16, output pitch 64 (got %d / %d)", c.Ci, c.Co);
  FFA_REQUIRE(c.Ho == (c.Hi - 1) / 2 + 1 && c.Wo == (c.Wi - 1) / 2 + 1,
              "stem conv: output size of a 7x7 stride-2 pad-3 convolution");
  FFA_REQUIRE((long long)StemGeom::IH * c.Wi * 32 < (1LL << 31), "stem conv: input tensor must be smaller than 2 GiB");
  r->kernel = FFA_CONV_KERNEL_STEM;
  r->variant = 0;
  r->th = StemGeom::TH;
  r->tw = StemGeom::TW;
  r->tiles_x = ffa_cdiv(c.Wo, r->tw);
  r->tiles_y = ffa_cdiv(c.Ho, r->th);
  r->ntiles = c.B * r->tiles_x * r->tiles_y;
  r->ncb = 1;
  int cap = 256;
  if (const char* e = getenv("FFA_STEM_GRID")) {
    const int v = atoi(e);
    if (v > 0) cap = v;
  }
  r->grid = r->ntiles < cap ? r->ntiles : cap;
  return 0;
}

// in [B][Hi][Wi][16] bf16 (channels >= 8 are never read; pad channels must be zero), out [B][Ho][Wo][64]
int ffa_stem_launch(const ffa_conv_call_t& c, const ffa_conv_route_t& r, hipStream_t stream) {
  StemArgs a;
  a.in = c.in; a.w = c.w; a.out = c.out; a.bias = c.bias; a.stats = c.stats;
  a.B = c.B; a.Hi = c.Hi; a.Wi = c.Wi; a.Ho = c.Ho; a.Wo = c.Wo; a.Co = c.Co; a.relu = c.relu;
  a.tiles_x = r.tiles_x;
  a.tiles_y = r.tiles_y;
  a.npt = r.ntiles;
  hipLaunchKernelGGL(conv7x7_stem_kernel, dim3(r.grid), dim3(StemGeom::NTHR), 0, stream, a);
  return ffa_check_launch("conv7x7_stem");
}
