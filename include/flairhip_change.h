/* libflairhip -- C ABI of land-cover change between two class rasters on one grid: per-zone class transitions and
 * change codes.  Part of flairhip.h, which includes this file inside its extern "C" block after flairhip_zonestats.h
 * (the zone tables and FFA_ZONE_STATS_* are that file's): include flairhip.h, not this file.  The conventions are
 * flairhip.h's.  The ctypes side is flairhip.lib.CHANGE_SIGNATURES (tests/test_change_abi_cpu.py compares the two). */
#ifndef FLAIRHIP_CHANGE_H
#define FLAIRHIP_CHANGE_H

#ifndef FLAIRHIP_H
#error "include flairhip.h: it declares the types this header uses and includes it"
#endif

#define FFA_CHANGE_MAX_CLASSES 32

/* Per-zone transition matrices: definition (normative).
 *
 * Inputs.  Two device uint8 class rasters before[H][W] and after[H][W] on one grid; optionally a device uint8
 * confidence raster conf[H][W] (the after run's); K in 1..FFA_CHANGE_MAX_CLASSES; Z zones.  The rings, the zones and
 * every host-provided table (xy_pix, ring_offsets, zone_ring_offsets, windows, plane_offsets, scan_starts, chunks) are
 * exactly those of ffa_zone_stats_u8 (flairhip_zonestats.h), with the same limits, and the workspace is the one
 * ffa_zone_stats_workspace_bytes sizes: the same layout, contents irrelevant on entry.
 *
 * Membership is bit for bit ffa_zone_stats_u8's: one host function builds the planes for both entry points.
 *
 * Outputs (device, written, not accumulated).  counts[Z][K + 1][K + 1], int64: counts[z][a][b] = the number of member
 * pixels of zone z with min(before, K) == a and min(after, K) == b; row and column K ("other") collect the values >= K,
 * such as the zone clip's 255.  With conf, conf_sums of the same shape: the sum of the conf bytes over the same pixels;
 * conf == NULL leaves conf_sums untouched (it may be NULL).  The sum of counts[z] over b is the counts row that
 * ffa_zone_stats_u8 gives for before, the sum over a the one for after.
 *
 * Atomics are integer only: equal inputs give equal bytes whatever the schedule.  The tables are not trusted: every
 * index derived from them is clamped to the raster or checked against plane_words, so a wrong table gives wrong
 * numbers, never an access outside a buffer.  No floating point in the tabulation; no host synchronisation; capturable.
 *
 * K is bounded by the per-wave tables of the tabulation: (K + 1)^2 uint32 for the counts and as many for the
 * confidence sums, four waves a block, 34848 bytes of static LDS at K = 32.  K outside 1..32 is FFA_ERR_ARG. */
int ffa_zone_change_u8(const uint8_t* before, const uint8_t* after, const uint8_t* conf, int H, int W, int K,
                       const double* xy_pix, long long n_vertices, const int32_t* ring_offsets, int n_rings,
                       const int32_t* zone_ring_offsets, int n_zones, const int32_t* windows,
                       const int64_t* plane_offsets, long long plane_words, const int64_t* scan_starts,
                       long long n_scan_items, const int32_t* chunks, long long n_chunks, int64_t* counts,
                       int64_t* conf_sums, void* ws, long long ws_bytes, ffa_stream_t stream);

/* Change codes: definition (normative).
 *
 * out[i] = lut[min(before[i], K) * (K + 1) + min(after[i], K)] for 0 <= i < n; before, after and out are device uint8
 * arrays of n bytes at any alignment, lut a device uint8 table of (K + 1)^2 bytes, K in 1..FFA_CHANGE_MAX_CLASSES
 * (else FFA_ERR_ARG), 0 <= n (n == 0 launches nothing).  out may be before or after itself (every byte is read before
 * the same lane writes it); any other overlap between out and an input is undefined.  No host synchronisation;
 * capturable. */
int ffa_change_code_u8(const uint8_t* before, const uint8_t* after, long long n, int K, const uint8_t* lut,
                       uint8_t* out, ffa_stream_t stream);

#endif /* FLAIRHIP_CHANGE_H */
