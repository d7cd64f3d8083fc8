/* libflairhip -- C ABI of object matching: the overlaps between the regions of two class rasters.  Part of flairhip.h,
 * which includes this file inside its extern "C" block after the types it needs (ffa_stream_t, FFA_ERR_*): include
 * flairhip.h, not this file.  The conventions are flairhip.h's.  The ctypes side is flairhip.lib.OBJECT_SIGNATURES
 * (tests/test_objects_cpu.py compares the two). */
#ifndef FLAIRHIP_OBJECTS_H
#define FLAIRHIP_OBJECTS_H

#ifndef FLAIRHIP_H
#error "include flairhip.h: it declares the types this header uses and includes it"
#endif

/* Definitions (normative).
 *
 * A region of a uint8 raster [H][W] is a 4-connected component of equal value: the polygoniser's meaning.  With
 * background >= 0 that value is no region; background = -1 makes every value a class.  A region's label is the
 * row-major index of its first pixel.  Regions with fewer than min_pixels pixels are dropped.  The kept regions of a
 * raster, in ascending label order, form its region table: first_pixel (int32), class (int32), pixels (int64), with
 * indices 0 .. P - 1.  A stable sort of that table by class is exactly the polygon order of ffa_polygonize_emit for
 * the same (classes, background, min_pixels): polygons are sorted by (class, label).  That is what lets a polygon
 * column be filled from a region index.
 *
 * The overlap list of rasters A and B of the same H, W is the set of triples (ia, ib, n): n > 0 is the number of
 * pixels lying in kept region ia of A and in kept region ib of B.  The class plays no role here; filtering by class
 * is the host's business.  The set is a function of the inputs alone, and all its numbers are exact integers.
 *
 * The pair bound Q.  A pixel has a pair when it lies in a kept region of both rasters.  It is a head when its left
 * neighbour does not exist (first column) or has no pair or a different pair, and its upper neighbour does not exist
 * (first row) or has no pair or a different pair.  Q is the number of heads.  It bounds the number of distinct pairs:
 * among the pixels of a 4-connected patch of one pair the row-major first one has neither a left nor an upper
 * neighbour in the patch, so it is a head, and every distinct pair has at least one patch.
 *
 * Two phases keep the ABI rules (no host synchronisation inside a call, caller workspace) although the output size
 * depends on the data; all calls on one stream, no floating point anywhere, integer vector atomics on global memory
 * only, no grid-wide barrier:
 *   1. ffa_region_overlap_count labels both rasters, numbers the kept regions of each in label order (a device-wide
 *      exclusive scan of the kept-root flags) and writes counts_dev[4] (int64, device memory): Pa, Pb, Q, 0.
 *      Its workspace ws of ffa_region_overlap_bytes(H, W) bytes holds, per raster, the region index of every pixel
 *      (-1: background or a dropped region), the pixel counts and the classes of the roots; about 22 bytes per pixel.
 *      Limit: H * W < 2^30 (FFA_ERR_ARG from both, with the numbers in ffa_last_error).
 *   2. the caller reads Pa, Pb and Q, allocates the outputs and a hash table of ffa_region_overlap_table_bytes(Q)
 *      bytes -- host only: capacity cap = the smallest power of two >= max(2 * Q, 64), uint64 keys[cap] followed by
 *      int64 n[cap] -- and calls ffa_region_overlap_pairs on the same workspace, untouched in between.  It fills the
 *      region tables a_first / a_class / a_pixels [Pa] and b_first / b_class / b_pixels [Pb], clears the table (keys
 *      all-ones, counts 0), inserts every pixel that has a pair under the key index_a << 32 | index_b (runs of equal
 *      keys inside a wave folded to one insertion; linear probing bounded by cap steps) and compacts the occupied
 *      slots into pair_a (int32), pair_b (int32) and pair_pixels (int64), each of length Q.  It writes
 *      counts_dev[3] = n_pairs and counts_dev[2] = 1 if the table overflowed, else 0 (with cap >= 2 * Q that cannot
 *      happen on correct code: the bound makes a defect an error code, not a hang); counts_dev[0] and [1] stay.
 *      Pa, Pb and Q must be the values step 1 wrote.
 * The first n_pairs entries of the pair arrays are the overlap list in unspecified order.  This is the one place
 * where the ABI does not promise equal bytes for equal inputs; the set and every number in it are deterministic.
 * (flairhip.ops.region_overlaps sorts the list by (ia, ib); after that sort equal inputs give equal bytes.)
 * With Pa == 0, Pb == 0 or Q == 0 there are no pairs: the table and the pair outputs are not touched and may be null,
 * nothing of the pair passes is launched; the region table of a side that has regions is still filled. */
long long ffa_region_overlap_bytes(int H, int W); /* < 0 (FFA_ERR_ARG) beyond the limit */
int ffa_region_overlap_count(const uint8_t* a, const uint8_t* b, int H, int W, int background_a, int background_b,
                             long long min_pixels_a, long long min_pixels_b, void* ws, long long ws_bytes,
                             long long* counts_dev, ffa_stream_t stream);
long long ffa_region_overlap_table_bytes(long long Q); /* < 0 (FFA_ERR_ARG) outside 0 <= Q < 2^30 */
int ffa_region_overlap_pairs(const void* ws, long long ws_bytes, int H, int W, long long Pa, long long Pb, long long Q,
                             void* table, long long table_bytes, int32_t* a_first, int32_t* a_class,
                             int64_t* a_pixels, int32_t* b_first, int32_t* b_class, int64_t* b_pixels,
                             int32_t* pair_a, int32_t* pair_b, int64_t* pair_pixels, long long* counts_dev,
                             ffa_stream_t stream);

#endif /* FLAIRHIP_OBJECTS_H */
