"""The LDS image of the attention train kernels' streamed tiles
(metaflow_amd/ops/csrc/attn_lds_image.h), checked on the CPU.

The header's addressing functions are pure integer constexpr code, so this
test compiles them for the host, dumps every address the three kernels
form, and checks:

* each image is a bijection of rows x 16 chunks onto the tile's bytes, and
  every lane address has the alignment its instruction needs;
* the lane-base + immediate split the kernels use equals ``off`` of the
  (row, chunk) the fragment comments promise, for the row read and for the
  transposed read, the latter run through the ds_read_b64_tr_b16 gather
  rule (lane 4q+p of a 16-lane group supplies row q, columns 4p..4p+3; lane
  i receives column i, row q in element q);
* under the LDS bank rules every row read and transposed read is
  conflict-free and the staging writes at most 2-way;
* the same bank model gives the 16-wide panel layout the figures its
  counters showed (2x, 2x, 4x, 2x), which is the model's self-check.

Bank rules (gfx950): ds_read_b128 is serviced in four fixed 16-lane groups
{0-3,12-15,20-27}, {4-11,16-19,28-31} and the same +32, 64 banks of 4
bytes; ds_read_b64_tr_b16 per 32-lane half, 64 banks; ds_write_b128 in
eight groups of 8 contiguous lanes, 32 banks. Lanes that touch the same
dword share one access; a group takes as many cycles as its busiest bank
holds distinct dwords.
"""

import json
import os
import shutil
import subprocess
from collections import defaultdict
from fractions import Fraction

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "metaflow_amd", "ops", "csrc")

ROWS = 64
TILE_BYTES = ROWS * 256

DUMP = r"""
#include <cstdio>
#include "attn_lds_image.h"
using namespace lds_img;
static_assert(off_a(0, 0) == 0, "constexpr on the host");
int main() {
  printf("{\"off_a\":[");
  for (int r = 0; r < 64; ++r) for (int c = 0; c < 16; ++c)
    printf("%s%d", r + c ? "," : "", off_a(r, c));
  printf("],\"off_b\":[");
  for (int r = 0; r < 64; ++r) for (int c = 0; c < 16; ++c)
    printf("%s%d", r + c ? "," : "", off_b(r, c));
  printf("],\"off_panel\":[");
  for (int r = 0; r < 64; ++r) for (int c = 0; c < 16; ++c)
    printf("%s%d", r + c ? "," : "", off_panel(64, r, c));
  printf("],\"row_base_a\":[");
  for (int l = 0; l < 64; ++l) for (int p = 0; p < 2; ++p)
    printf("%s%d", l + p ? "," : "", row_base_a(l, p));
  printf("],\"row_imm_a\":[");
  for (int t = 0; t < 2; ++t) for (int s = 0; s < 8; ++s)
    printf("%s%d", t + s ? "," : "", row_imm_a(t, s));
  printf("],\"row_addr_a\":[");
  for (int l = 0; l < 64; ++l) for (int t = 0; t < 2; ++t)
    for (int s = 0; s < 8; ++s)
      printf("%s%d", l + t + s ? "," : "", row_addr_a(l, t, s));
  printf("],\"tr_base_a\":[");
  for (int l = 0; l < 64; ++l) for (int u = 0; u < 2; ++u)
    printf("%s%d", l + u ? "," : "", tr_base_a(l, u));
  printf("],\"tr_imm_a\":[");
  for (int k = 0; k < 4; ++k) for (int n = 0; n < 4; ++n)
    printf("%s%d", k + n ? "," : "", tr_imm_a(k, n));
  printf("],\"tr_addr_a\":[");
  for (int l = 0; l < 64; ++l) for (int k = 0; k < 4; ++k)
    for (int n = 0; n < 4; ++n) for (int u = 0; u < 2; ++u)
      printf("%s%d", l + k + n + u ? "," : "", tr_addr_a(l, k, n, u));
  printf("],\"stage16_addr_a\":[");
  for (int i = 0; i < 1024; ++i)
    printf("%s%d", i ? "," : "", stage16_addr_a(i));
  printf("],\"stage16_rc\":[");
  for (int i = 0; i < 1024; ++i)
    printf("%s%d", i ? "," : "", stage16_row(i) * 16 + stage16_ch(i));
  printf("],\"stage_walk_addr_a\":[");
  for (int i = 0; i < 1024; ++i)
    printf("%s%d", i ? "," : "", stage_walk_addr_a(64, i));
  printf("],\"stage_walk_rc\":[");
  for (int i = 0; i < 1024; ++i)
    printf("%s%d", i ? "," : "",
           stage_walk_row(64, i) * 16 + stage_walk_ch(64, i));
  printf("]}\n");
  return 0;
}
"""


def _host_compiler():
    for name in ("c++", "g++", "clang++"):
        path = shutil.which(name)
        if path:
            return [path]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if os.path.exists(hipcc):
        return [hipcc, "-x", "c++"]
    return None


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cc = _host_compiler()
    if cc is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("lds_image")
    src = tmp / "dump.cpp"
    src.write_text(DUMP)
    exe = tmp / "dump"
    proc = subprocess.run(cc + ["-std=c++17", "-O1", "-I", CSRC, str(src),
                                "-o", str(exe)],
                          capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True,
                         check=True).stdout
    return json.loads(out)


# ---------------------------------------------------------------- the model
B128_GROUPS = [
    [0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
    [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31],
]
B128_GROUPS = B128_GROUPS + [[l + 32 for l in g] for g in B128_GROUPS]
TR_GROUPS = [list(range(0, 32)), list(range(32, 64))]
WRITE_GROUPS = [list(range(g * 8, g * 8 + 8)) for g in range(8)]


def _cycles(addrs, groups, nbytes, banks):
    """LDS-array cycles of one wave instruction: per service group, the
    largest number of distinct dwords that fall into one bank."""
    total = 0
    for grp in groups:
        per_bank = defaultdict(set)
        for lane in grp:
            for w in range(nbytes // 4):
                dword = addrs[lane] // 4 + w
                per_bank[dword % banks].add(dword)
        total += max(len(v) for v in per_bank.values())
    return total


def _ratio(instrs, groups, nbytes, banks):
    """cycles of a list of wave instructions relative to conflict-free"""
    cyc = sum(_cycles(a, groups, nbytes, banks) for a in instrs)
    return Fraction(cyc, len(instrs) * len(groups))


def row_ratio(instrs):
    return _ratio(instrs, B128_GROUPS, 16, 64)


def tr_ratio(instrs):
    return _ratio(instrs, TR_GROUPS, 8, 64)


def write_ratio(instrs):
    return _ratio(instrs, WRITE_GROUPS, 16, 32)


# --------------------------------------------- the kernels' maps, any image
def row_read_instrs(off):
    """row read: lane 32hi+l32 takes chunk 2s+hi of row 32t+l32"""
    return [[off(32 * t + (l & 31), 2 * s + (l >> 5)) for l in range(64)]
            for t in range(2) for s in range(8)]


def tr_rc(lane, ks, n, u):
    """(row, chunk, byte in chunk) lane supplies for fragment n, read u of
    k-step ks: block rows 16ks + 8hi + 4u .., columns 32n + 16g .."""
    hi, g, q, p = lane >> 5, (lane >> 4) & 1, (lane >> 2) & 3, lane & 3
    return 16 * ks + 8 * hi + 4 * u + q, 4 * n + 2 * g + (p >> 1), 8 * (p & 1)


def tr_read_instrs(off):
    out = []
    for ks in range(4):
        for n in range(4):
            for u in range(2):
                a = []
                for l in range(64):
                    r, c, b = tr_rc(l, ks, n, u)
                    a.append(off(r, c) + b)
                out.append(a)
    return out


def stage16_instrs(off):
    """512 threads, slot idx = u*512 + tid: chunk idx%16 of row idx//16"""
    return [[off((u * 512 + w * 64 + l) // 16, (u * 512 + w * 64 + l) % 16)
             for l in range(64)] for u in range(2) for w in range(8)]


def stage_walk_instrs(off):
    """512 threads, slot idx = it*512 + tid: chunk idx//64 of row idx%64"""
    return [[off((u * 512 + w * 64 + l) % 64, (u * 512 + w * 64 + l) // 64)
             for l in range(64)] for u in range(2) for w in range(8)]


def _off_fn(table):
    return lambda r, c: table[r * 16 + c]


# -------------------------------------------------------------------- tests
@pytest.mark.parametrize("image", ["off_a", "off_b", "off_panel"])
def test_image_is_a_bijection(dump, image):
    offs = dump[image]
    assert len(offs) == ROWS * 16
    assert sorted(offs) == list(range(0, TILE_BYTES, 16))


def test_row_read_delivers_its_fragment(dump):
    """base + immediate == off_a(32t + l32, 2s + hi), 16-byte aligned"""
    off = _off_fn(dump["off_a"])
    for l in range(64):
        for t in range(2):
            for s in range(8):
                addr = (dump["row_base_a"][l * 2 + (s & 1)]
                        + dump["row_imm_a"][t * 8 + s])
                assert addr == dump["row_addr_a"][(l * 2 + t) * 8 + s]
                assert addr % 16 == 0
                assert addr == off(32 * t + (l & 31), 2 * s + (l >> 5)), (
                    l, t, s)
    # immediates fit the DS offset field next to any lane base
    assert max(dump["row_imm_a"]) + max(dump["row_base_a"]) < TILE_BYTES


def test_transposed_read_delivers_its_fragment(dump):
    """Run the hardware gather over the lanes' addresses: lane 32hi + l32
    must receive rows 16ks + 8hi + 4u + (0..3) of column 32n + l32."""
    where = {}  # byte offset of a chunk -> (row, chunk)
    for r in range(ROWS):
        for c in range(16):
            where[dump["off_a"][r * 16 + c]] = (r, c)
    for ks in range(4):
        for n in range(4):
            for u in range(2):
                addr = []
                for l in range(64):
                    a = (dump["tr_base_a"][l * 2 + u]
                         + dump["tr_imm_a"][ks * 4 + n])
                    assert a == dump["tr_addr_a"][
                        ((l * 4 + ks) * 4 + n) * 2 + u]
                    assert a % 8 == 0
                    addr.append(a)
                for l in range(64):
                    grp, i = l // 16, l % 16
                    hi, l32 = l >> 5, l & 31
                    for q in range(4):
                        byte = addr[16 * grp + 4 * q + (i >> 2)] + 2 * (i & 3)
                        row, ch = where[byte & ~15]
                        col = ch * 8 + (byte & 15) // 2
                        assert (row, col) == (16 * ks + 8 * hi + 4 * u + q,
                                              32 * n + l32), (ks, n, u, l, q)
    assert max(dump["tr_imm_a"]) + max(dump["tr_base_a"]) < TILE_BYTES


def test_header_maps_match_the_generic_forms(dump):
    """The header's per-lane functions are the generic maps applied to
    off_a, so the bank figures below speak about the kernels' addresses."""
    off = _off_fn(dump["off_a"])
    rows = row_read_instrs(off)
    for t in range(2):
        for s in range(8):
            assert rows[t * 8 + s] == [
                dump["row_addr_a"][(l * 2 + t) * 8 + s] for l in range(64)]
    trs = tr_read_instrs(off)
    for ks in range(4):
        for n in range(4):
            for u in range(2):
                assert trs[(ks * 4 + n) * 2 + u] == [
                    dump["tr_addr_a"][((l * 4 + ks) * 4 + n) * 2 + u]
                    for l in range(64)]
    flat = [a for ins in stage16_instrs(off) for a in ins]
    assert flat == dump["stage16_addr_a"]
    flat = [a for ins in stage_walk_instrs(off) for a in ins]
    assert flat == dump["stage_walk_addr_a"]


@pytest.mark.parametrize("kind", ["stage16", "stage_walk"])
def test_staging_covers_the_tile_once(dump, kind):
    assert sorted(dump[kind + "_rc"]) == list(range(ROWS * 16))
    assert sorted(dump[kind + "_addr_a"]) == list(range(0, TILE_BYTES, 16))
    off = dump["off_a"]
    assert [off[rc] for rc in dump[kind + "_rc"]] == dump[kind + "_addr_a"]


def test_bank_model_reproduces_the_panel_layout(dump):
    """self-check of the model: the panel layout's measured figures"""
    off = _off_fn(dump["off_panel"])
    assert row_ratio(row_read_instrs(off)) == 2
    assert tr_ratio(tr_read_instrs(off)) == 2
    assert write_ratio(stage16_instrs(off)) == 4
    assert write_ratio(stage_walk_instrs(off)) == 2


def test_image_a_reads_conflict_free_writes_two_way(dump):
    """image A, used by the forward, dQ and dK/dV: every single read
    instruction conflict-free, every staging write at most 2-way"""
    off = _off_fn(dump["off_a"])
    for a in row_read_instrs(off):
        assert _cycles(a, B128_GROUPS, 16, 64) == len(B128_GROUPS)
    for a in tr_read_instrs(off):
        assert _cycles(a, TR_GROUPS, 8, 64) == len(TR_GROUPS)
    for instrs in (stage16_instrs(off), stage_walk_instrs(off)):
        for a in instrs:
            for grp in WRITE_GROUPS:
                assert _cycles(a, [grp], 16, 32) <= 2
    assert write_ratio(stage16_instrs(off)) == 2
    assert write_ratio(stage_walk_instrs(off)) == 2


def test_image_b_figures_of_the_header_table(dump):
    """image B is not used; the header's comparison table quotes it"""
    off = _off_fn(dump["off_b"])
    assert row_ratio(row_read_instrs(off)) == 1
    assert tr_ratio(tr_read_instrs(off)) == 1
    assert write_ratio(stage16_instrs(off)) == 1
    assert write_ratio(stage_walk_instrs(off)) == 2
