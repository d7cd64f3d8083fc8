/* libflairhip -- C ABI of calibrated class thresholds.  Part of flairhip.h, which includes this file inside its
 * extern "C" block after the types it needs (ffa_stream_t, FFA_BF16 / FFA_F32, FFA_ERR_*): include flairhip.h, not this
 * file.  The conventions are flairhip.h's.  The ctypes side is flairhip.lib.CALIB_SIGNATURES (tests/test_calib_abi_cpu.py
 * compares the two). */
#ifndef FLAIRHIP_CALIB_H
#define FLAIRHIP_CALIB_H

#ifndef FLAIRHIP_H
#error "include flairhip.h: it declares the types this header uses and includes it"
#endif

/* Definitions.
 *
 * Score byte.  For a pixel with logits z[0..K): m = maximum, e_k = expf(z_k - m), se = sum of e_k in class order,
 * q_k = (uint8) rintf(e_k / se * 255.f): bit for bit the byte ffa_predict_u8 mode 1 writes for class k at that pixel.
 *
 * Score histograms.  hist[k][s][q], int64 [K][2][256], accumulating like ffa_confusion_matrix's counts: for every pixel
 * with target t < K and every class k, hist[k][t == k ? 1 : 0][q_k] += 1.  A pixel with t >= K contributes nowhere (the
 * rule of ffa_eval_stats).  Counts are integers: equal inputs give equal bytes in any schedule.
 *
 * Thresholded label.  Given thr[0..K) (uint8) and fallback (uint8): class k passes when q_k >= thr[k]; the label is
 * the passing class with the greatest z_k, the lowest index on a tie (the strict '>' of mode 0, restricted to passing
 * classes); if no class passes the label is fallback.  With all thresholds 0 the label plane equals mode 0 byte for
 * byte.
 *
 * Confidence plane (the analogue of mode 2).  q of the chosen class; 0 where the label is fallback because nothing
 * passed.
 *
 * TTA path.  On an accumulator, p_k = acc_k / (float)views, q_k = rintf(p_k * 255.f) and the ordering is on p_k: the
 * arithmetic of ffa_tta_predict_u8. */

/* hist += the score histograms of NHWC logits [npix][Cp] (bf16 / f32, K real classes, the constraints of
 * ffa_eval_stats, 16-byte aligned) against uint8 targets.  npix <= 2^31 (a block-local 32-bit bin cannot overflow);
 * npix == 0 is a no-op.  No floating-point atomics, no host synchronisation; capturable. */
int ffa_calib_hist(int dtype, const void* logits, const uint8_t* targets, long long npix, int K, int Cp,
                   long long* hist, ffa_stream_t stream);
/* ffa_predict_u8 with thresholds (thr: device, K bytes): mode 0 -> out [B][h][w] thresholded labels; mode 2 -> out
 * [B][2][h][w], label plane and confidence plane.  Mode 1 is refused: thresholds do not apply to class-probability
 * output.  The constraints of ffa_predict_u8; fallback in 0..255.  No host synchronisation; capturable. */
int ffa_predict_thresholded_u8(int dtype, int mode, const void* logits, const uint8_t* thr, int fallback, uint8_t* out,
                               int B, int H, int W, int K, int Cp, int y0, int x0, int h, int w, ffa_stream_t stream);
/* The same two outputs from an accumulator of `views` views (the constraints of ffa_tta_predict_u8).  With one identity
 * view they equal ffa_predict_thresholded_u8's bit for bit. */
int ffa_tta_predict_thresholded_u8(int mode, const float* acc, const uint8_t* thr, int fallback, uint8_t* out, int B,
                                   int K, int Cp, int h, int w, int views, ffa_stream_t stream);

#endif /* FLAIRHIP_CALIB_H */
