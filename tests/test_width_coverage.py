"""tests/widths.py reaches every width-instantiation the six fused loss sources build.  MAX_NDT, MAX_NK and MAX_NF are read out
of the sources, so raising one of them fails here until the width lists are extended; each source is credited only with the
widths its own GPU file ran before (widths.OLD_GRID), so a width whose instantiation nothing else launches cannot go; and the
lists are held to the stated tuples element by element, so deleting ANY width fails — also one whose NDT another width of the
list reaches as well (96 beside 72, 160 beside 130: the unpadded and the padded form of the same instantiation)."""
import os
import re

import pytest

from tests import widths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "id-grec_amd", "csrc")
NDT_SOURCES = {"idg_mixnce.hip": "IDG_MIX_CASE", "idg_sccf.hip": "IDG_SCCF_CASE", "idg_nance.hip": "IDG_NA_CASE",
               "idg_svdnce.hip": "IDG_SVD_CASE"}  # the macro that instantiates the source's tile kernels per NDT


def _constant(source, name):
    found = re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, open(os.path.join(CSRC, source)).read())
    assert len(found) == 1, (source, name, found)
    return int(found[0])


def _cases(source, macro):
    """The arguments of the source's IDG_*_CASE(n)-style instantiation list."""
    return {int(n) for n in re.findall(r"\b%s\((\d+)\)" % macro, open(os.path.join(CSRC, source)).read())}


def test_the_lists_are_the_stated_ones():
    """Width by width: a deleted, added or changed entry fails, whatever else still reaches its instantiation."""
    assert widths.EVERY_NDT == (32, 72, 96, 128, 130, 160, 192, 200, 224, 256)
    assert widths.EVERY_NK == (96, 160, 192, 224)
    assert widths.NF3_WIDTH == 192
    assert widths.LIGHTGCL_CHUNKED == (96, 128, 160, 224)
    assert widths.B_TILES == (129, 257)
    assert set(widths.LIGHTGCL_CHUNKED) <= set(widths.EVERY_NDT) and widths.NF3_WIDTH in widths.EVERY_NK
    assert [widths.ndt(d) for d in widths.EVERY_NDT] == [1, 3, 3, 4, 5, 5, 6, 7, 7, 8]
    assert [d for d in widths.EVERY_NDT if d % 32] == [72, 130, 200]  # the widths with padding columns


@pytest.mark.parametrize("source", sorted(NDT_SOURCES))
def test_every_ndt_is_reached(source):
    max_ndt = _constant(source, "MAX_NDT")
    old = {widths.ndt(d) for d in widths.OLD_GRID[source]}
    new = {widths.ndt(d) for d in widths.EVERY_NDT}
    assert new | old == set(range(1, max_ndt + 1)), (source, sorted(new | old))
    assert max(widths.EVERY_NDT) == 32 * max_ndt
    # the new list alone reaches every value this source's old grid left out
    assert set(range(1, max_ndt + 1)) - old <= new, (source, sorted(set(range(1, max_ndt + 1)) - old - new))
    # the source instantiates exactly 1 .. MAX_NDT
    built = _cases(source, NDT_SOURCES[source])
    assert built == set(range(1, max_ndt + 1)), (source, sorted(built))


def test_lightgcl_is_credited_with_its_tile_pass_widths_only():
    """LightGCL's older cases above SMALL_B ran NDT 1, 2 and 8: NDT 3 .. 7 — d = 128 among them — hang on EVERY_NDT alone."""
    small_b = _constant("idg_svdnce.hip", "SMALL_B")
    assert small_b == 127 and min(widths.B_TILES) > small_b
    assert {widths.ndt(d) for d in widths.OLD_GRID["idg_svdnce.hip"]} == {1, 2, 8}
    for d in (128,) + widths.LIGHTGCL_CHUNKED:
        assert widths.ndt(d) not in {widths.ndt(o) for o in widths.OLD_GRID["idg_svdnce.hip"]}
    assert {widths.ndt(d) for d in widths.LIGHTGCL_CHUNKED} == {3, 4, 5, 7}


def test_every_nk_is_reached():
    max_nk = _constant("idg_vae.hip", "MAX_NK")
    assert all(d % 32 == 0 for d in widths.EVERY_NK + widths.OLD_GRID["idg_vae.hip"])
    old = {d // 32 for d in widths.OLD_GRID["idg_vae.hip"]}
    assert old == {1, 2, 4, 8}
    new = {d // 32 for d in widths.EVERY_NK}
    assert new | old == set(range(1, max_nk + 1)), sorted(new | old)
    assert set(range(1, max_nk + 1)) - old <= new
    for macro in ("IDG_NLL_STATS", "IDG_NLL_GRAD"):
        assert _cases("idg_vae.hip", macro) == set(range(1, max_nk + 1)), macro


def test_nf_3_is_reached():
    max_nf = _constant("idg_au.hip", "MAX_NF")
    assert widths.NF3_WIDTH % 64 == 0 and widths.NF3_WIDTH // 64 == 3 <= max_nf
    old = {d // 64 for d in widths.OLD_GRID["idg_au.hip"]}
    assert old == {1, 2, 4} and old | {widths.NF3_WIDTH // 64} == set(range(1, max_nf + 1))
