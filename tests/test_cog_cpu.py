"""Cloud-optimised GeoTIFF writer, validator and overview reader of flair_zonal_detection/geotiff.py (no GPU: the
levels come from the numpy oracle of the overview definition).  All comparisons are exact."""
import hashlib

import numpy as np
import pytest

from flair_zonal_detection.geotiff import GeoTiffError, GeoTiffRaster, GeoTiffWriter, validate_cog, write_cog
from overview_oracle import n_levels, pyramid

LEFT, TOP, RES = 651992.4, 6860417.8, 0.2


def _levels(bands, H, W, block, method="mode", seed=3):
    g = np.random.default_rng(seed)
    base = g.integers(0, 19, (bands, H, W), dtype=np.uint8)
    return [base] + pyramid(base, n_levels(H, W, block), method)


def _check_file(p, levels, block, compress):
    assert validate_cog(p) == []
    with GeoTiffRaster(p) as r:
        assert r.overview_count == len(levels) - 1
        assert np.array_equal(r.read(), levels[0])
        assert r.res == (RES, RES) and r.crs == "EPSG:2154"
        b, (_, H, W) = r.bounds, levels[0].shape
        assert (b.left, b.top, b.right, b.bottom) == (LEFT, TOP, LEFT + W * RES, TOP - H * RES)
        assert r.profile["tiled"] and r.profile["blockxsize"] == block and r.profile["blockysize"] == block
        assert r.profile["compress"] == compress
        assert r.profile["interleave"] == ("band" if levels[0].shape[0] > 1 else "pixel")
    for k in range(1, len(levels)):
        with GeoTiffRaster(p, overview=k) as r:
            _, h, w = levels[k].shape
            assert (r.count, r.height, r.width) == levels[k].shape
            assert np.array_equal(r.read(), levels[k])
            assert r.res == (RES * 2 ** k, RES * 2 ** k) and r.crs == "EPSG:2154"
            b = r.bounds
            assert (b.left, b.top) == (LEFT, TOP)
            assert (b.right, b.bottom) == (LEFT + w * RES * 2 ** k, TOP - h * RES * 2 ** k)
            assert r.overview_count == len(levels) - 1
    with pytest.raises(GeoTiffError, match="overview"):
        GeoTiffRaster(p, overview=len(levels))


@pytest.mark.parametrize("compress", [None, "lzw", "deflate"])
@pytest.mark.parametrize("bands", [1, 3])
def test_ragged_raster_with_several_levels_reads_back(tmp_path, bands, compress):
    levels = _levels(bands, 37, 53, 16)
    assert [lv.shape[1:] for lv in levels] == [(37, 53), (19, 27), (10, 14)]  # ragged edge tiles on every level
    p = str(tmp_path / "cog.tif")
    assert write_cog(p, levels, LEFT, TOP, RES, crs="EPSG:2154", blocksize=16, compress=compress) == p
    _check_file(p, levels, 16, compress)


@pytest.mark.parametrize("bands", [1, 3])
def test_raster_within_one_block_has_no_overviews(tmp_path, bands):
    levels = _levels(bands, 30, 32, 32)
    assert len(levels) == 1
    p = str(tmp_path / "small.tif")
    write_cog(p, levels, LEFT, TOP, RES, crs="EPSG:2154", blocksize=32)
    _check_file(p, levels, 32, "lzw")


def test_default_blocksize_and_average_levels(tmp_path):
    levels = _levels(1, 600, 1030, 512, method="average")
    assert [lv.shape[1:] for lv in levels] == [(600, 1030), (300, 515), (150, 258)]
    p = str(tmp_path / "avg.tif")
    write_cog(p, levels, LEFT, TOP, (RES, RES), crs="EPSG:2154", nodata=255)
    _check_file(p, levels, 512, "lzw")
    with GeoTiffRaster(p, overview=2) as r:
        assert r.nodata == 255.0


def test_layout_ifds_first_then_smallest_overview_first(tmp_path):
    import struct
    levels = _levels(3, 37, 53, 16)
    p = str(tmp_path / "cog.tif")
    write_cog(p, levels, LEFT, TOP, RES, crs="EPSG:2154", blocksize=16)
    raw = open(p, "rb").read()
    assert raw[:4] == b"II*\0" and struct.unpack_from("<I", raw, 4)[0] == 8
    from flair_zonal_detection.geotiff import _parse_ifd
    off, tags = 8, []
    while off:
        t, nxt = _parse_ifd(raw, "<", False, off)
        tags.append((off, t))
        assert nxt == 0 or nxt > off
        off = nxt
    assert len(tags) == 3
    assert 254 not in tags[0][1] and 33550 in tags[0][1] and 34735 in tags[0][1]
    for _, t in tags[1:]:
        assert t[254] == (1,) and not any(k in t for k in (33550, 33922, 34735, 34736, 34737))
    for _, t in tags:
        assert t[322] == (16,) and t[323] == (16,) and t[284] == (2,)
        assert list(t[324]) == sorted(t[324])  # band, tile row, tile column in file order
    firsts = [t[324][0] for _, t in tags]
    assert firsts[2] < firsts[1] < firsts[0]
    assert max(t[324][-1] + t[325][-1] for _, t in tags[1:]) <= firsts[0]
    assert tags[2][1][324][-1] + tags[2][1][325][-1] <= firsts[1]


def test_validator_rejects_a_plain_geotiff_and_bad_files(tmp_path):
    g = np.random.default_rng(5)
    p = str(tmp_path / "plain.tif")

    class Small(GeoTiffWriter):
        BLOCK = 16

    w = Small(p, 53, 37, 1, LEFT, TOP, RES, crs="EPSG:2154")
    w.data[:] = g.integers(0, 19, (1, 37, 53), dtype=np.uint8)
    w.close()
    errors = validate_cog(p)
    assert any("no overviews" in e for e in errors)
    assert any("directly after" in e for e in errors)
    assert any("does not lie before the first pixel data" in e for e in errors)
    # a file of one block with its IFD at the end is still refused; the same raster through write_cog passes
    q = str(tmp_path / "one.tif")
    w = Small(q, 16, 16, 1, LEFT, TOP, RES)
    w.close()
    assert validate_cog(q) and not any("no overviews" in e for e in validate_cog(q))
    junk = tmp_path / "junk.tif"
    junk.write_bytes(b"not a tiff")
    assert validate_cog(str(junk)) == ["not a TIFF file"]


def test_validator_sees_misordered_overviews(tmp_path):
    levels = _levels(1, 37, 53, 16)
    p = str(tmp_path / "bad.tif")
    with pytest.raises(GeoTiffError, match="does not follow"):
        write_cog(p, [levels[0], levels[2], levels[1]], LEFT, TOP, RES, blocksize=16)
    with pytest.raises(GeoTiffError, match="blocksize"):
        write_cog(p, levels, LEFT, TOP, RES, blocksize=100)
    with pytest.raises(GeoTiffError, match="compress"):
        write_cog(p, levels, LEFT, TOP, RES, blocksize=16, compress="jpeg")
    # swap the tile offset arrays' order on disk: point overview 1's first tile behind the main image's
    import struct
    write_cog(p, levels, LEFT, TOP, RES, blocksize=16, compress=None)
    raw = bytearray(open(p, "rb").read())
    from flair_zonal_detection.geotiff import _parse_ifd
    t0, nxt = _parse_ifd(raw, "<", False, 8)
    # find overview 1's TileOffsets entry and overwrite its out-of-line array with offsets past the main image's
    (n,) = struct.unpack_from("<H", raw, nxt)
    for k in range(n):
        e = nxt + 2 + 12 * k
        tag, _, cnt, voff = struct.unpack_from("<HHII", raw, e)
        if tag == 324:
            far = t0[324][-1]
            struct.pack_into("<" + "I" * cnt, raw, voff, *([far] * cnt))
    q = tmp_path / "swapped.tif"
    q.write_bytes(bytes(raw))
    assert any("smaller overviews must come first" in e for e in validate_cog(str(q)))


def _pillow_reads_tiled_lzw(tmp_path):
    """whether this Pillow can write and re-read a multi-page tiled LZW TIFF of ITS OWN (libtiff built in): decided on
    Pillow's file, never on the file under test"""
    from PIL import Image, features
    if not features.check("libtiff"):
        return False
    own = str(tmp_path / "pillow_own.tif")
    pages = [Image.fromarray(np.arange(40 * 48, dtype=np.uint8).reshape(40, 48) % 19),
             Image.fromarray(np.arange(20 * 24, dtype=np.uint8).reshape(20, 24) % 19)]
    try:
        pages[0].save(own, compression="tiff_lzw", save_all=True, append_images=pages[1:],
                      tiffinfo={322: 16, 323: 16})
        with Image.open(own) as im:
            back = []
            for k in range(2):
                im.seek(k)
                back.append(np.asarray(im).copy())
    except Exception:
        return False
    return all(np.array_equal(x, np.asarray(y)) for x, y in zip(back, pages))


def test_pillow_reads_every_page(tmp_path):
    Image = pytest.importorskip("PIL.Image", reason="Pillow is the independent TIFF implementation of these tests")
    if not _pillow_reads_tiled_lzw(tmp_path):
        pytest.skip("this Pillow has no libtiff that reads its own multi-page LZW TIFF")
    levels = _levels(1, 37, 53, 16)
    p = str(tmp_path / "cog.tif")
    write_cog(p, levels, LEFT, TOP, RES, crs="EPSG:2154", blocksize=16)
    with Image.open(p) as im:  # from here on every Pillow error is a failure of the file write_cog made
        assert im.n_frames == len(levels)
        for k in range(len(levels)):
            im.seek(k)
            assert np.array_equal(np.asarray(im), levels[k][0]), k


def test_validator_reports_directories_without_sizes(tmp_path):
    import struct
    levels = _levels(1, 37, 53, 16)
    p = str(tmp_path / "cog.tif")
    write_cog(p, levels, LEFT, TOP, RES, blocksize=16, compress=None)
    raw = bytearray(open(p, "rb").read())
    nowidth = bytearray(raw)
    (n,) = struct.unpack_from("<H", nowidth, 8)
    for k in range(n):  # rename ImageWidth of IFD 0 to an unknown private tag (kept in tag order: 256 -> 255)
        if struct.unpack_from("<H", nowidth, 10 + 12 * k)[0] == 256:
            struct.pack_into("<H", nowidth, 10 + 12 * k, 255)
    q = tmp_path / "nowidth.tif"
    q.write_bytes(bytes(nowidth))
    assert any("ImageWidth" in e for e in validate_cog(str(q)))
    noifd = bytearray(raw)
    struct.pack_into("<I", noifd, 4, 0)
    q = tmp_path / "noifd.tif"
    q.write_bytes(bytes(noifd))
    assert any("no image directory" in e for e in validate_cog(str(q)))


def test_foreign_overviews_masks_are_skipped_and_resolution_follows_the_size(tmp_path):
    """a mask overview (NewSubfileType 5, as GDAL writes) is no overview of the image; an overview whose size is not
    ceil(size / 2^k) gets its resolution from the size ratio"""
    import struct
    base = np.random.default_rng(9).integers(0, 19, (1, 48, 64), dtype=np.uint8)
    odd = base[:, ::3, ::4].copy()  # 16 x 16: a factor 3 down, 4 across
    p = str(tmp_path / "foreign.tif")
    write_cog(p, [base, odd, odd[:, ::2, ::2].copy()], LEFT, TOP, RES, crs="EPSG:2154", blocksize=16, compress=None)
    with GeoTiffRaster(p, overview=1) as r:
        assert r.shape == (16, 16) and r.res == (RES * 4, RES * 3) and np.array_equal(r.read(), odd)
        assert tuple(r.bounds) == tuple(GeoTiffRaster(p).bounds)
    raw = bytearray(open(p, "rb").read())
    from flair_zonal_detection.geotiff import _parse_ifd
    _, nxt = _parse_ifd(raw, "<", False, 8)
    (n,) = struct.unpack_from("<H", raw, nxt)
    for k in range(n):
        e = nxt + 2 + 12 * k
        if struct.unpack_from("<H", raw, e)[0] == 254:
            struct.pack_into("<I", raw, e + 8, 5)  # reduced-resolution + transparency mask
    q = tmp_path / "mask.tif"
    q.write_bytes(bytes(raw))
    with GeoTiffRaster(str(q)) as r:
        assert r.overview_count == 1
    with GeoTiffRaster(str(q), overview=1) as r:
        assert r.shape == (8, 8)


# SHA-256 of the files GeoTiffWriter.close() wrote BEFORE its encoder and IFD packing were factored out for write_cog
# (recorded from the parent commit's code on the array below); Deflate is left out: its bytes depend on the zlib build.
PARENT_SHA256 = {
    (1, "lzw"): "4583fdb7a5db2eeefb83213521f54c588de5b1bc40458946ae774cd68762d238",
    (1, "none"): "a2e10c915de26c8c77e5774baaf8945909efb6949f92986ca4eb792465e4a900",
    (3, "lzw"): "93abde073cba17dfff6121a797abe99cf6be91d47be93f17fbe8d368d00d38ca",
    (3, "none"): "962215705b0c5ae21153bc216cf75db603fafc9b9473ee67c9c80780d24eead2",
}


@pytest.mark.parametrize("bands,compress", sorted(PARENT_SHA256))
def test_plain_writer_bytes_are_those_of_the_parent_commit(tmp_path, bands, compress):
    data = np.random.default_rng(20261018).integers(0, 19, (bands, 300, 421), dtype=np.uint8)
    p = str(tmp_path / "plain.tif")
    w = GeoTiffWriter(p, 421, 300, bands, 700000.0, 6600000.0, 0.2, crs="EPSG:2154", compress=compress, nodata=255)
    w.data[:] = data
    w.close()
    assert hashlib.sha256(open(p, "rb").read()).hexdigest() == PARENT_SHA256[(bands, compress)]
    with GeoTiffRaster(p) as r:  # a plain file: no overviews, reads as before
        assert r.overview_count == 0 and np.array_equal(r.read(), data)


def test_convert_to_cog_refuses_to_overwrite_its_input(tmp_path):
    """a name the '.tif' -> '_COG.tif' rule leaves unchanged (upper-case suffix) must not end with the only copy deleted;
    refused before anything is read or written, so no GPU is needed"""
    from flair_zonal_detection.postprocess import convert_to_cog
    p = str(tmp_path / "PRED.TIF")
    w = GeoTiffWriter(p, 40, 30, 1, LEFT, TOP, RES)
    w.close()
    before = open(p, "rb").read()
    assert p.replace(".tif", "_COG.tif") == p
    with pytest.raises(ValueError, match="other than its input"):
        convert_to_cog(p, p.replace(".tif", "_COG.tif"))
    with pytest.raises(ValueError, match="other than its input"):
        convert_to_cog(p, str(tmp_path / "sub" / ".." / "PRED.TIF"))
    assert open(p, "rb").read() == before


def test_equal_inputs_give_equal_files(tmp_path):
    levels = _levels(3, 37, 53, 16)
    a, b = str(tmp_path / "a.tif"), str(tmp_path / "b.tif")
    write_cog(a, levels, LEFT, TOP, RES, crs="EPSG:2154", blocksize=16)
    write_cog(b, [lv.copy() for lv in levels], LEFT, TOP, RES, crs="EPSG:2154", blocksize=16)
    assert open(a, "rb").read() == open(b, "rb").read()
