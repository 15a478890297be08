"""CPU: the L2-group tile order of the NT GEMM kernels (csrc/tile_order.h), compiled as plain host C++ -- the plan on the shapes whose group
counts the GPU tests rely on, and the decoder (rounded-up reciprocals + one compare) against the division form on every position: equal
coordinates, a bijection onto the tile grid, n-fastest inside a group.  The same program may be built with -fsanitize=address,undefined and run
by hand; that is not part of the suite."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

CLANG = os.path.join(kr.LLVM, "clang++")
pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the LLVM clang++")

PROGRAM = r"""
#include "tile_order.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

// plan: tiles_m tiles_n BN K N l2_kib single_kib -> "ngroup last_width groups"
// walk: tiles_m tiles_n BN K N l2_kib single_kib -> checks every position, prints "ok <positions>" or the first failure
int main(int argc, char **argv)
{
    if (argc != 9) return 2;
    int a[7];
    for (int i = 0; i < 7; ++i) a[i] = atoi(argv[2 + i]);
    const TileOrder o = tile_order_plan(a[0], a[1], a[2], a[3], a[4], a[5], a[6]);
    const int groups = (o.tiles_n + o.ngroup - 1) / o.ngroup;
    if (argv[1][0] == 'p') {
        printf("%d %d %d\n", o.ngroup, o.tiles_n - (groups - 1) * o.ngroup, groups);
        return 0;
    }
    const int total = o.tiles_m * o.tiles_n;
    std::vector<char> seen((size_t)total, 0);
    int ptm = -1, ptn = -1, pg = -1;
    for (int pos = 0; pos < total; ++pos) {
        int tm, tn;
        tile_order_coords(o, pos, tm, tn);
        // the division form
        const int full = o.ngroup * o.tiles_m, g = pos / full, r = pos - g * full;
        const int gsize = (g + 1) * o.ngroup <= o.tiles_n ? o.ngroup : o.tiles_n - g * o.ngroup;
        const int dm = r / gsize, dn = g * o.ngroup + (r - dm * gsize);
        if (tm != dm || tn != dn) { printf("pos %d: (%d, %d), division form (%d, %d)\n", pos, tm, tn, dm, dn); return 1; }
        if (tm < 0 || tm >= o.tiles_m || tn < 0 || tn >= o.tiles_n || seen[(size_t)tm * o.tiles_n + tn]++) { printf("pos %d: (%d, %d) outside the grid or twice\n", pos, tm, tn); return 1; }
        // n-fastest inside a group: the next position is the next n-tile of the group, or the group's first n-tile one m-row down
        if (g == pg && !((tm == ptm && tn == ptn + 1) || (tm == ptm + 1 && tn == g * o.ngroup && ptn == g * o.ngroup + gsize - 1))) { printf("pos %d: (%d, %d) after (%d, %d)\n", pos, tm, tn, ptm, ptn); return 1; }
        if (g != pg && (tm != 0 || tn != g * o.ngroup)) { printf("pos %d: group %d starts at (%d, %d)\n", pos, g, tm, tn); return 1; }
        ptm = tm; ptn = tn; pg = g;
    }
    printf("ok %d\n", total);
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("tile_order")
    src, exe = d / "tile_order_check.cpp", d / "tile_order_check"
    src.write_text(PROGRAM)
    subprocess.run([CLANG, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "emdr2_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    return str(exe)


def _run(program, mode, tiles_m, tiles_n, BN, K, N, l2_kib=2560, single_kib=4096):
    out = subprocess.run([program, mode] + [str(v) for v in (tiles_m, tiles_n, BN, K, N, l2_kib, single_kib)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.split()


@pytest.mark.parametrize("name,args,want", [
    ("11 n-tiles of 256, K 768, N 2816: room for 6, 6 + 5", (18, 11, 256, 768, 2816), (6, 5, 2)),
    ("N 3080, K 64: 385 KiB <= 4 MiB, one group", (18, 13, 256, 64, 3080), (13, 13, 1)),
    ("9 n-tiles with room for 6: 5 + 4, not 6 + 3", (16, 9, 256, 768, 2304, 2560, 1024), (5, 4, 2)),
    ("the same 9 n-tiles under the 4 MiB rule (N K 2 = 3.4 MiB): one group", (16, 9, 256, 768, 2304, 2560, 4096), (9, 9, 1)),
    ("2 ng < tiles_n (room for 1 of 12, K 3072): one group", (16, 12, 256, 3072, 3072), (12, 12, 1)),
])
def test_plan(program, name, args, want):
    assert tuple(int(v) for v in _run(program, "plan", *args)) == want, name


@pytest.mark.parametrize("name,args,groups", [
    ("12,800 x 6 in one group (the reciprocal of 76,800 is one too large from tile 59,075 on)", (12800, 6, 256, 3072, 1536, 2560, 1 << 30), 1),
    ("18 x 11 in groups of 6 + 5", (18, 11, 256, 768, 2816), 2),
    ("13 x 10 in one group", (13, 10, 256, 64, 2312), 1),
    ("13 x 10 in groups of 5 + 5", (13, 10, 256, 1024, 2560), 2),
    ("a single n-tile", (193, 1, 256, 32, 136), 1),
    ("a single m-tile: one group, where 2 groups of ONE tile each would have fit", (1, 2, 256, 8192, 512), 1),
])
def test_decoder_matches_the_division_form_on_every_position(program, name, args, groups):
    assert int(_run(program, "plan", *args)[2]) == groups, name
    assert _run(program, "walk", *args) == ["ok", str(args[0] * args[1])], name
