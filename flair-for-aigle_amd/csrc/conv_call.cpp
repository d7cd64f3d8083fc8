// The convolution call: generic checks, the form x layout table and the two ABI entries (conv_call.h).
#include "conv_call.h"

// The one router: ffa_conv_route answers with it, ffa_conv_run launches what it says.
static int conv_route(const ffa_conv_call_t& c, ffa_conv_route_t* r) {
  FFA_REQUIRE(c.dtype == FFA_BF16 || c.dtype == FFA_F32, "conv: bad dtype %d", c.dtype);
  FFA_REQUIRE(c.form == FFA_CONV_PLAIN || c.form == FFA_CONV_UPCAT || c.form == FFA_CONV_POOLED, "conv: bad form %d", c.form);
  FFA_REQUIRE(c.B > 0 && c.Hi > 0 && c.Wi > 0 && c.Ho > 0 && c.Wo > 0, "conv: bad dims");
  FFA_REQUIRE(c.Ci % 16 == 0 && c.Co % 8 == 0, "conv: channel pitch must be a multiple of 16 (in) / 8 (out), got %d/%d", c.Ci, c.Co);
  FFA_REQUIRE(c.dil == 1 || c.dil == 2, "conv: dil must be 1 or 2");
  FFA_REQUIRE(c.dil == 1 || c.stride == 1, "conv: zero-insertion input needs stride 1");
  FFA_REQUIRE((c.pro_scale == nullptr) == (c.pro_shift == nullptr), "conv: prologue needs scale and shift");
  FFA_REQUIRE(!c.bnx || (c.stats && c.bn_scale && c.bn_shift), "conv_bnbwd: null pointer");
  FFA_REQUIRE(!c.bnx || (!c.bias && !c.relu), "conv_bnbwd: the output is a gradient (no bias, no relu)");
  const bool same = c.kh == 3 && c.kw == 3 && c.stride == 1 && c.pad == 1 && c.dil == 1 && c.Hi == c.Ho && c.Wi == c.Wo;
  if (c.form == FFA_CONV_UPCAT) {
    FFA_REQUIRE(same && c.Hi % 2 == 0 && c.Wi % 2 == 0 && c.c1 > 0 && c.c1 <= c.Ci && c.c1 % 16 == 0, "conv_upcat: bad dims");
    FFA_REQUIRE(!c.residual && !c.bnx, "conv_upcat: no residual input in the upsampled form");
  } else if (c.form == FFA_CONV_POOLED) {
    FFA_REQUIRE(same && c.Ho % 2 == 0 && c.Wo % 2 == 0 && c.c1 > 0 && c.c1 <= c.Co && c.c1 % 8 == 0, "dgrad_upcat: bad dims");
    FFA_REQUIRE(!c.bias && !c.residual && !c.relu && !c.stats && !c.pro_scale && !c.bnx,
                "conv: the pooled form has a plain epilogue");
  }
  if (c.form != FFA_CONV_UPCAT)  // (the two-source form has two stored inputs: its layout's route checks them)
    FFA_REQUIRE((long long)c.B * c.Hi * c.Wi * c.Ci * ffa_conv_elem_bytes(c.dtype) < (1LL << 31),
                "conv: input tensor must be smaller than 2 GiB (32-bit piece offsets)");

  // Which layout serves which form (the table of include/flairhip.h); the family's route function then holds the call
  // to the geometry its layout was packed for.
  const int layout = c.bco & (FFA_BCO_RING | FFA_BCO_THIN | FFA_BCO_STEM);
  const bool ring = layout == FFA_BCO_RING, thin = layout == FFA_BCO_THIN, stem = layout == FFA_BCO_STEM;
  FFA_REQUIRE(layout == 0 || ring || thin || stem, "conv: bad operand layout 0x%x", c.bco);
  if (c.pro_scale && !(thin || (ring && c.form == FFA_CONV_PLAIN))) {
    ffa_set_error("conv_pro: no prologue kernel for this operand layout (bco 0x%x, form %d)", c.bco, c.form);
    return FFA_ERR_UNSUPPORTED;
  }
  if (c.form != FFA_CONV_PLAIN && (ring || stem)) {
    ffa_set_error("conv: a ring- or stem-layout operand serves the plain form only");
    return FFA_ERR_UNSUPPORTED;
  }
  if (stem) return ffa_stem_route(c, r);
  if (thin) return ffa_thin_route(c, r);
  if (ring) return ffa_ring_route(c, r);
  return ffa_igemm_route(c, r);
}

extern "C" int ffa_conv_route(const ffa_conv_call_t* call, ffa_conv_route_t* route) {
  FFA_REQUIRE(call && route, "conv: null pointer");
  return conv_route(*call, route);
}

extern "C" int ffa_conv_run(const ffa_conv_call_t* call, ffa_stream_t stream) {
  FFA_REQUIRE(call, "conv: null pointer");
  const ffa_conv_call_t& c = *call;
  FFA_REQUIRE(c.in && c.w && c.out, "conv: null pointer");
  FFA_REQUIRE(c.form != FFA_CONV_UPCAT || c.in2 || c.c1 == c.Ci, "conv_upcat: null pointer");
  FFA_REQUIRE(c.form != FFA_CONV_POOLED || c.out2 || c.c1 == c.Co, "dgrad_upcat: null pointer");
  ffa_conv_route_t r;
  const int rc = conv_route(c, &r);
  if (rc != 0) return rc;
  switch (r.kernel) {
    case FFA_CONV_KERNEL_STEM: return ffa_stem_launch(c, r, stream);
    case FFA_CONV_KERNEL_THIN: return ffa_thin_launch(c, r, stream);
    case FFA_CONV_KERNEL_RING:
    case FFA_CONV_KERNEL_RING16: return ffa_ring_launch(c, r, stream);
    default: return ffa_igemm_launch(c, r, stream);
  }
}

extern "C" int ffa_conv_struct_bytes(int which) {
  return which == 0 ? (int)sizeof(ffa_conv_call_t) : (int)sizeof(ffa_conv_route_t);
}

extern "C" int ffa_conv_upcat_supported(int dtype, int c1, int c2) {
  return (dtype == FFA_BF16 || dtype == FFA_F32) && c1 > 0 && c2 >= 0 && c1 % 16 == 0 && c2 % 16 == 0 &&
         ffa_igemm_upcat_split_ok(dtype, c1, c2) && ffa_wgrad_upcat_split_ok(dtype, c1, c2);
}
