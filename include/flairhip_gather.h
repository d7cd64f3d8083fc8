/* libflairhip -- C ABI of the device-resident sample store.  Part of flairhip.h, which includes this file inside its
 * extern "C" block after the types it needs (ffa_stream_t, FFA_BF16 / FFA_F32, FFA_SRC_*, FFA_ERR_*): include
 * flairhip.h, not this file.  The conventions are flairhip.h's.  The ctypes side is flairhip.lib.GATHER_SIGNATURES
 * (tests/test_gather_abi_cpu.py compares the two). */
#ifndef FLAIRHIP_GATHER_H
#define FLAIRHIP_GATHER_H

#ifndef FLAIRHIP_H
#error "include flairhip.h: it declares the types this header uses and includes it"
#endif

/* elevation pre-processing of a 2-band DEM_ELEV sample (band 0 = surface model z0, band 1 = terrain model z1) */
#define FFA_ELEV_NONE 0  /* channels as stored */
#define FFA_ELEV_DIFF 1  /* one channel z0 - z1 (flair_hub/data/utils_data/elevation.py:11 calc_elevation) */
#define FFA_ELEV_STACK 2 /* two channels (z0, z0 - z1) (flair_hub/data/dataloader.py:140-141 calc_elevation_stack_dsm) */

/* Image b of the NHWC output [B][H][W][Cp] (dtype FFA_BF16 / FFA_F32) is image index[b] of the raw NCHW store
 * [N][C_src][H][W] (src_kind FFA_SRC_*), read through the gather of ffa_d4_nchw_to_nhwc (codes[b / group]) and
 * normalised (x - mean[c]) / stdv[c]; pad channels are zero.  index: int32 [B] on the device (a captured step replays
 * with new indices).  codes null: the identity, and H != W is then allowed.  mean and stdv both null: FFA_SRC_F32 only.
 * elevation FFA_ELEV_DIFF / FFA_ELEV_STACK need C_src == 2; the difference is taken in the sample type widened to f32,
 * before the normalisation, and mean / stdv are indexed by OUTPUT channel (1 resp. 2 entries).  Cp % 8 == 0 and Cp >=
 * the output channel count.  With FFA_ELEV_NONE the output is bit-identical to ffa_d4_nchw_to_nhwc on the gathered
 * images.  An index outside [0, N) is a caller error: the kernel clamps it and never reads outside the store. */
int ffa_gather_layout(int dtype, int src_kind, const void* store, const int* index, void* dst, int N, int B, int C_src,
                      int H, int W, int Cp, const float* mean, const float* stdv, const uint8_t* codes, int group,
                      int elevation, ffa_stream_t stream);
/* uint8 label store [N][H][W] -> uint8 class indices [B][H][W] through the same gather (codes[b], or null).  The label
 * rule is the reference's argmax(reshape_label_ohe(label, K)) (label.py:12-14, tasks_module.py:153): a value v < K
 * stays v; a value v >= K becomes 0 -- its one-hot is all false and the argmax of that is 0.  1 <= num_classes <= 256. */
int ffa_gather_labels_u8(const uint8_t* store, const int* index, uint8_t* dst, int N, int B, int H, int W,
                         int num_classes, const uint8_t* codes, ffa_stream_t stream);

#endif /* FLAIRHIP_GATHER_H */
