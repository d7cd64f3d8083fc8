/* libflairhip -- C ABI of the evaluation stage.  Part of flairhip.h, which includes this file inside its extern "C"
 * block after the types it needs (ffa_stream_t, FFA_BF16 / FFA_F32, FFA_ERR_*): include flairhip.h, not this file.
 * The conventions are flairhip.h's.  The ctypes side is flairhip.lib.EVAL_SIGNATURES (tests/test_eval_abi_cpu.py
 * compares the two). */
#ifndef FLAIRHIP_EVAL_H
#define FLAIRHIP_EVAL_H

#ifndef FLAIRHIP_H
#error "include flairhip.h: it declares the types this header uses and includes it"
#endif

/* Everything an evaluation needs from NHWC logits [npix][Cp] (bf16 / f32, K real classes, the constraints of
 * ffa_softmax_ce, 16-byte aligned) and uint8 targets, in one pass (flair_hub/tasks/tasks_module.py:280-335 per-class
 * validation loss and IoU; flair_hub/writer/prediction_writer.py labels + confusion matrix).  A target >= K
 * contributes to nothing.
 *   pred[i]        = the first maximum over k < K: the bytes of ffa_softmax_ce's pred
 *   confmat[t][p] += 1 for t < K (int64, rows = target, accumulating like ffa_confusion_matrix)
 *   class_count[k] = number of pixels with target k (int64, overwritten)
 *   class_nll[k]   = sum over those pixels of (log sum_j exp(z_j) - z_k), unweighted (float64, overwritten); the
 *                    per-pixel term in f32 as ffa_softmax_ce computes it (maximum m, expf(z_j - m) summed in class
 *                    order, logf of the sum) minus (z_k - m) -- finite however far z_k lies below the maximum --,
 *                    summed in a fixed order: per thread, per block (f32 partials in the workspace), then over the
 *                    blocks in double.
 * pred, confmat and the pair (class_nll, class_count) may each be null and are then skipped (the workspace is needed
 * for the pair only).  No floating-point atomics: equal inputs give equal bytes.  No host synchronisation; capturable.
 * npix == 0 writes zeros. */
long long ffa_eval_stats_workspace_bytes(void);
int ffa_eval_stats(int dtype, const void* logits, const uint8_t* targets, long long npix, int K, int Cp,
                   uint8_t* pred, long long* confmat, double* class_nll, long long* class_count, void* workspace,
                   long long workspace_bytes, ffa_stream_t stream);

#endif /* FLAIRHIP_EVAL_H */
