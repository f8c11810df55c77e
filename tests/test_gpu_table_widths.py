"""The Huffman table builders on crafted histograms at every width, byte for byte
against the oracle.

Both builders choose their code by the number n of present symbols of a table:
the fused tail of k_hist (tables_tail: tail_levels<1|2|4|8> for n <= 32, <= 64,
<= 128 and above, in <8> a second register pair for the package masks, the
two-slot sort for an AC table of n <= 128, sort_bitonic<4> above, the one-slot DC
sort) and the k_tables launch (galloping merges in LDS; stripes, frames past
tables_fusable's bound, DMMT_FUSE_TABLES=0).  Image content reaches those widths
by accident only, so the frames here are coefficient blocks built for a wanted
histogram (tests/tools/hist_blocks.py) and go through encode_coefficients; the
cases and their preconditions are in tests/tools/table_width_cases.py:

  * luma AC tables of 1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129 and 241
    symbols (241: every usable symbol, ZRL and EOB included), the chroma AC table
    of another width class in the same launch, each with
      - every count the same, and two counts interleaved over the symbol values
        (the stable order by symbol decides the file);
      - from 31 symbols: a chain of heavy symbols over a bulk of rare ones, the
        unlimited Huffman tree deeper than 15, the oracle's longest code 16;
      - from 31 symbols: the same with (0, 15) the least frequent symbol -- a
        16-bit code and 15 extra bits, the longest piece k_emit is given -- in the
        first, a middle and the last block of a chunk of 256 blocks and in a
        block of more than kSlotWords * 32 = 384 bits (the re-walk);
    and 33, 129 and 241 symbols with the chain at 4:2:0 (four luma blocks per MCU);
  * DC tables of 1, 2, 12 and 16 categories, the 16 with every count the same and
    with Fibonacci counts (a 16-bit DC code), and a category-15 difference that
    carries the 16-bit code in the last and the first block of a chunk (no restart
    interval) and in the MCU behind a restart marker (intervals 1 and 7, where a
    chunk starts with every segment; DC values stay within +-16383, so the block
    right behind the marker has category 14 at most and the next one carries it).

Every case asserts its preconditions on the oracle's file and the builder's own
histogram first (symbols per table, the longest code in BITS, the unlimited depth
above 15, the least frequent symbol and its length, the block count stated here);
tests/test_hist_blocks.py asserts the same without a GPU.  Then the fused tables
and a DMMT_FUSE_TABLES=0 context must both give the oracle's bytes.

Not here: the 64-bit keys (tail_rank<1|2|4>, a frequency of 2^24 or more) need a
frame of 2^24 symbols and stay with test_gpu_fused_edges.py's
test_fused_tables_u64_keys.
[length_limited.rs:37-134, symbol_counting.rs:55-94, huffman/encoder.rs:45-157,
encoder.rs:356-404]"""
import os
import sys

import pytest

import dmmt_jpeg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import table_width_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def unfused():
    """a context whose tables come from the k_tables launch"""
    os.environ["DMMT_FUSE_TABLES"] = "0"
    try:
        enc = dmmt_jpeg.Encoder(0)
    finally:
        os.environ.pop("DMMT_FUSE_TABLES")
    yield enc
    enc.close()


@pytest.mark.parametrize("name", cases.NAMES)
def test_table_widths(encoder, unfused, name):
    case = cases.make(name)
    ref = cases.reference(name)
    assert case.coef.shape[0] == cases.BLOCKS[name]
    cases.check(case, ref)
    luma, chroma = dmmt_jpeg.quality_tables(90)
    opts = dmmt_jpeg.JpegTransformationOptions(dmmt_jpeg.ChromaSubsamplingPreset(case.sub), 8, luma_table=luma,
                                              chroma_table=chroma, restart_interval=case.restart_interval)
    for which, enc in (("fused tables", encoder), ("k_tables", unfused)):
        got = enc.encode_coefficients(case.coef, case.width, case.height, opts)
        assert got == ref, f"{name}, {which}: the file differs from the oracle's"
