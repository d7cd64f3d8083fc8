/* libflairhip -- C ABI of zonal statistics: per-zone class areas and confidence sums.  Part of flairhip.h, which includes
 * this file inside its extern "C" block after the types it needs (ffa_stream_t, FFA_ERR_*): include flairhip.h, not
 * this file.  The conventions are flairhip.h's.  The ctypes side is flairhip.lib.ZONESTATS_SIGNATURES
 * (tests/test_zonestats_abi_cpu.py compares the two). */
#ifndef FLAIRHIP_ZONESTATS_H
#define FLAIRHIP_ZONESTATS_H

#ifndef FLAIRHIP_H
#error "include flairhip.h: it declares the types this header uses and includes it"
#endif

/* Definition (normative).
 *
 * Inputs.  A device uint8 class raster cls[H][W]; optionally a device uint8 confidence raster conf[H][W] on the same
 * grid; K in 1..256; Z zones.  Rings arrive as for ffa_zone_mask_u8: float64 pixel coordinates xy_pix[V][2], int32
 * ring_offsets[R + 1] (ring_offsets[R] = V), rings need not be closed and may have either orientation.  Zone z owns the
 * rings zone_ring_offsets[z] .. zone_ring_offsets[z + 1] - 1 (int32 [Z + 1], zone_ring_offsets[Z] = R).
 *
 * Membership.  Pixel (r, c) belongs to zone z when its centre is inside, even-odd over all rings of z.  The crossing
 * rule is exactly ffa_zone_mask_u8's (flairhip.h, "geozone clipping", the four bullets): the same separately rounded
 * float64 expression for xc, the same column floor(xc - 0.5) + 1, edges with a non-finite coordinate ignored; one device
 * function (csrc/ffa_zone.h) serves both.  The member pixels of one zone are therefore bit for bit the mask that
 * ffa_zone_mask_u8 gives for that zone's rings in one call.  Zones are independent and may overlap: a pixel counts in
 * every zone that contains it.  A valid MultiPolygon is one zone holding the rings of all its parts.
 *
 * Outputs (device, written, not accumulated).  counts[Z][K + 1], int64: counts[z][k] = the number of pixels of zone z
 * with cls == k for k < K; column K ("other") collects the pixels with cls >= K, such as the zone clip's 255.  With
 * conf, conf_sums[Z][K + 1], int64: the sum of the conf bytes over the same pixels; conf == NULL leaves conf_sums
 * untouched (it may be NULL).  Atomics are integer only: equal inputs give equal bytes whatever the schedule.
 *
 * Host-provided tables (device memory; the kernels do not trust them: every index derived from them is clamped to the
 * raster or checked against plane_words, so a wrong table gives wrong numbers, never an access outside a buffer).
 *   windows[Z][4], int32 (r0, c0, r1, c1): the rows r0 .. r1 - 1 and columns c0 .. c1 - 1 that may hold pixels of the
 *     zone, clamped to the raster, c0 a multiple of 32.  The conservative rule from the zone's bounds in pixels:
 *       r0 = max(0, floor(ymin - 0.5)), r1 = min(H, ceil(ymax - 0.5) + 1),
 *       c0 = max(0, floor(xmin - 0.5)) & ~31, c1 = min(W, floor(xmax - 0.5) + 2).
 *     A crossing left of c0 toggles local column 0, one at or beyond c1 has no effect, rows outside [r0, r1) are
 *     skipped.  Each zone has its own bit plane uint32 [r1 - r0][ww], ww = ceil((c1 - c0) / 32); bit b of word w of a
 *     row is column c0 + 32 w + b.
 *   plane_offsets[Z], int64: the word offset of each zone's plane in one packed array of plane_words words.
 *   scan_starts[Z + 1], int64: the exclusive scan of the row-scan work items per zone; a zone with
 *     ww <= FFA_ZONE_STATS_NARROW_WORDS has ceil((r1 - r0) / 64) items (a lane per row), a wider one r1 - r0 (a wave
 *     per row, with the carry across more than 64 words).
 *   chunks[n_chunks][3], int32 (zone, first word, words): the work list of the tabulation, a wave each; words of one
 *     zone's plane, at most FFA_ZONE_STATS_CHUNK_WORDS per chunk (a per-wave 32-bit partial sum is bounded by
 *     255 * 32 * FFA_ZONE_STATS_CHUNK_WORDS < 2^32), every word of every plane in exactly one chunk.
 *
 * Limits.  V < 2^31 - 1, Z and R < 2^31, a zone's plane < 2^31 words, plane_words and every offset int64; the caller
 * bounds plane_words per call by its memory budget and splits the zones into several calls beyond it.
 *
 * The workspace (ffa_zone_stats_workspace_bytes, contents irrelevant on entry) holds the planes and the per-edge
 * tables of the span pass.  No floating point in the tabulation; no host synchronisation; capturable. */

#define FFA_ZONE_STATS_CHUNK_WORDS 2048
#define FFA_ZONE_STATS_NARROW_WORDS 8

/* < 0 (FFA_ERR_ARG) on bad arguments.  n_chunks takes no room (the chunk list is the caller's buffer); it is checked
 * against the range ffa_zone_stats_u8 accepts. */
long long ffa_zone_stats_workspace_bytes(long long n_vertices, long long plane_words, long long n_chunks);
int ffa_zone_stats_u8(const uint8_t* cls, const uint8_t* conf, int H, int W, int K, const double* xy_pix,
                      long long n_vertices, const int32_t* ring_offsets, int n_rings, const int32_t* zone_ring_offsets,
                      int n_zones, const int32_t* windows, const int64_t* plane_offsets, long long plane_words,
                      const int64_t* scan_starts, long long n_scan_items, const int32_t* chunks, long long n_chunks,
                      int64_t* counts, int64_t* conf_sums, void* ws, long long ws_bytes, ffa_stream_t stream);

#endif /* FLAIRHIP_ZONESTATS_H */
