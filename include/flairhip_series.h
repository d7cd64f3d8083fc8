/* libflairhip -- C ABI of the ragged time-series store.  Part of flairhip.h, which includes this file inside its
 * extern "C" block after flairhip_gather.h and the types it needs (ffa_stream_t, FFA_BF16 / FFA_F32, FFA_SRC_*,
 * FFA_ERR_*): include flairhip.h, not this file.  The conventions are flairhip.h's.  The ctypes side is
 * flairhip.lib.SERIES_SIGNATURES (tests/test_series_store_cpu.py compares the two). */
#ifndef FLAIRHIP_SERIES_H
#define FLAIRHIP_SERIES_H

#ifndef FLAIRHIP_H
#error "include flairhip.h: it declares the types this header uses and includes it"
#endif

/* The padded batch of a U-TAE branch from a ragged store.  data: [D][C][H][W] raw samples (src_kind FFA_SRC_*), the
 * dates of all N samples back to back; offsets: int32 [N + 1], the dates of sample i are offsets[i] .. offsets[i+1];
 * is_pad: uint8 [D], 1 where the stored date is constant at the model's pad value.  dst: NHWC [B*T][H][W][Cp] (dtype
 * FFA_BF16 / FFA_F32), pad: uint8 [B*T]; image b*T + t is date t of sample s = index[b].
 *   t <  len(s): the stored date read through the gather of ffa_d4_nchw_to_nhwc (codes[b]; null: the identity, and
 *                H != W is then allowed), widened to f32 and converted to dtype -- no normalisation, the reference
 *                normalises no series; pad channels zero; pad = is_pad[offsets[s] + t].
 *   t >= len(s): real channels hold `fill` (the 0 pad_collate_flair pads with), pad channels zero; pad = tail_is_pad
 *                (the host passes fill == pad_value).
 * Bit-identical to ffa_d4_nchw_to_nhwc(group = T) and ffa_detect_pad_images on the f32 [B*T][C][H][W] tensor
 * pad_collate_flair builds.  len(s) > T is a caller error: the dates beyond T are dropped.  An index outside [0, N) is
 * a caller error: the kernel clamps it.  index, offsets, is_pad and codes are read on the device (a captured step
 * replays with new indices); T is the only batch-dependent launch parameter.  Cp % 8 == 0 and Cp >= C. */
int ffa_gather_series(int dtype, int src_kind, const void* data, const int* offsets, const uint8_t* is_pad,
                      const int* index, void* dst, uint8_t* pad, int N, int B, int T, int C, int H, int W, int Cp,
                      float fill, int tail_is_pad, const uint8_t* codes, ffa_stream_t stream);

#endif /* FLAIRHIP_SERIES_H */
