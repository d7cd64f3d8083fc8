// One forward / input-gradient convolution call (ffa_conv_call_t) and the kernel families that serve it.
//
// conv_call.cpp holds the router: the generic checks and the table of which operand layout serves which form.  Each
// family file holds one route function -- the only place where that family's tile geometry, grid cap and eligibility
// for a form live; it makes no HIP call -- and one launcher, which fills the family's kernel-argument struct from the
// call and its route.  Queries (ffa_conv_route) and launches (ffa_conv_run) go through the same route function.
#pragma once
#include "ffa_common_host.h"

static inline int ffa_conv_elem_bytes(int dtype) { return dtype == FFA_BF16 ? 2 : 4; }

int ffa_igemm_route(const ffa_conv_call_t& c, ffa_conv_route_t* r);  // conv_igemm.hip
int ffa_igemm_launch(const ffa_conv_call_t& c, const ffa_conv_route_t& r, ffa_stream_t stream);
int ffa_ring_route(const ffa_conv_call_t& c, ffa_conv_route_t* r);   // conv3x3_ring.hip
int ffa_ring_launch(const ffa_conv_call_t& c, const ffa_conv_route_t& r, ffa_stream_t stream);
int ffa_thin_route(const ffa_conv_call_t& c, ffa_conv_route_t* r);   // conv3x3_thin.hip
int ffa_thin_launch(const ffa_conv_call_t& c, const ffa_conv_route_t& r, ffa_stream_t stream);
int ffa_stem_route(const ffa_conv_call_t& c, ffa_conv_route_t* r);   // conv7x7_stem.hip
int ffa_stem_launch(const ffa_conv_call_t& c, const ffa_conv_route_t& r, ffa_stream_t stream);

// layer eligibility for the thin / stem layouts (ffa_conv_plan)
bool ffa_thin_takes_layer(int dtype, int kh, int kw, int stride, int rows_real, int ci_pitch);
bool ffa_stem_takes_layer(int dtype, int kh, int kw, int stride, int cout, int ci_pitch);

// the two rules on the channel split of a two-source convolution (ffa_conv_upcat_supported)
bool ffa_igemm_upcat_split_ok(int dtype, int c1, int c2);  // conv_igemm.hip: c1 covers whole halo channel groups
bool ffa_wgrad_upcat_split_ok(int dtype, int c1, int c2);  // conv_wgrad.hip: c1 is a multiple of a block's input channels
