"""The model's `mtile` (look-ups and inserts alternate per sub-tile inside a tile) on the CPU alone: what the device option of the same name is compared with."""
import os

from conftest import ROOT


def test_model_sub_tiles_pay_on_source_code_and_round_trip(codec):
    with open(os.path.join(ROOT, "portable-network-archive_amd", "csrc", "k_zdec.hip"), "rb") as f:
        source = f.read()
    syn = [codec.corpus_file(0, i, 1 << 20) for i in (0, 1)]
    size = {}
    for mtile in (0, 2048, 1024, 512, 256):
        p = codec.params_for_level(3)
        p.mtile = mtile
        o = codec.model_compress(source, p)
        assert codec.zstd_decompress(o, len(source)) == source, mtile
        size["source", mtile] = len(o)
        size["syn", mtile] = sum(len(codec.model_compress(d, p)) for d in syn) if mtile in (0, 256) else 0
    assert size["source", 256] <= 0.90 * size["source", 0]                 # (27 174 / 31 762 = 0.856 when this was written)
    assert size["source", 256] <= size["source", 1024] <= size["source", 0]
    assert size["syn", 256] <= size["syn", 0]                               # (733 145 / 736 848)
    pd = codec.params_for_level(6, deflate=True)
    d0 = len(codec.deflate_model_compress(source, pd))
    pd.mtile = 256
    o = codec.deflate_model_compress(source, pd)
    import zlib
    assert zlib.decompress(o) == source and len(o) <= 0.90 * d0             # (29 628 / 34 879 = 0.849)
