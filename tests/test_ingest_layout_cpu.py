"""No GPU: the slot blob of a device-built sequence of more than 64 frames (csrc/pd_ggs_ingest_layout.h, the layout the ingest_nf_* kernels
index) compiled into a stand-alone host program under AddressSanitizer and UBSan: arrays in order, 256-byte aligned and disjoint, the
total equal to the formula the header documents, nothing truncated in `int` at the largest sizes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "posediffusion_amd", "csrc")

_PROGRAM = r"""
#include "pd_ggs_ingest_layout.h"
#include <stdio.h>
#include <vector>
static size_t al(size_t v) { return (v + 255) / 256 * 256; }
static int check(long long M, int N, long long P, long long I) {
    PdIngestNfLayout L;
    pd_ingest_nf_layout(M, N, P, I, L);
    const size_t m = (size_t)M, n = (size_t)N, p = (size_t)P, it = (size_t)I, tiles = (m + 1023) / 1024;
    /* (offset, bytes the kernels index) in blob order */
    const size_t a[][2] = {{L.pts, 16 * m}, {L.pij, 8 * p}, {L.pio, 4 * (p + 1)}, {L.itm, 16 * it}, {L.gps, 8 * p}, {L.gio, 4 * (n + 1)},
                           {L.cnt, 4 * (n * n + 1)}, {L.pex, 4 * (n * n + 1)}, {L.crk, 4 * n * n}, {L.keys, 4 * m}, {L.src, 4 * m},
                           {L.hist, 4 * 257 * tiles}, {L.btot, 4 * 257}};
    const int k = (int)(sizeof(a) / sizeof(a[0]));
    if (a[0][0] != 0) return 1;
    size_t sum = 0;
    for (int i = 0; i < k; ++i) {
        if (a[i][0] % 256) return 2;                                      /* aligned */
        const size_t next = i + 1 < k ? a[i + 1][0] : L.total;
        if (next <= a[i][0] || a[i][0] + a[i][1] > next) return 3;        /* ordered, disjoint */
        if (next - (a[i][0] + a[i][1]) >= 256) return 4;                  /* no slack beyond the alignment */
        sum += al(a[i][1]);
    }
    if (sum != L.total || L.total % 256) return 5;                        /* the documented formula */
    if (pd_ing_tiles(M) != tiles) return 6;
    /* scratch: 8 bytes per match, 12 per key, 1 028 per tile (+ alignment) */
    const size_t scratch = L.total - L.cnt, want = 8 * m + 12 * n * n + 8 + 1028 * tiles + 1028;
    if (scratch < want || scratch > want + 8 * 256) return 7;
    return 0;
}
int main() {
    const long long grid[][4] = {{16711680, 256, 65280, 65280}, {1, 1, 1, 1}, {16640, 65, 2080, 2080}, {16640, 65, 4225, 4225},
                                 {2147483647LL, 256, 65536, 65536}, {9792000, 256, 32640, 32640}, {1024, 65, 1, 1}, {1025, 100, 9900, 9900},
                                 {29700, 100, 10000, 10000}, {33024, 129, 16641, 16641}, {1023, 255, 7, 7}};
    for (const auto &g : grid) {
        const int rc = check(g[0], (int)g[1], g[2], g[3]);
        if (rc) {
            printf("M=%lld N=%lld P=%lld: rule %d\n", g[0], g[1], g[2], rc);
            return 1;
        }
    }
    /* nothing wraps in `int`: 32 640 pairs x 512 matches at 256 frames, and the most matches a sequence may hold (2^31 - 1: 32 GiB of pts) */
    PdIngestNfLayout L;
    pd_ingest_nf_layout(16711680, 256, 65280, 65280, L);
    if (L.pij != (size_t)16711680 * 16 || L.cnt - L.gio != al(4 * 257) || L.total != (size_t)420997120) return 2;
    pd_ingest_nf_layout(2147483647LL, 256, 65536, 65536, L);
    if (L.pij != ((size_t)1 << 35) || L.src - L.keys != ((size_t)1 << 33) || L.total <= ((size_t)48 << 30)) return 3;
    /* index the blob as the kernels do, on a small case, under the sanitizer */
    pd_ingest_nf_layout(3000, 65, 2080, 2080, L);
    std::vector<char> blob(L.total);
    int *hist = (int *)(blob.data() + L.hist), *btot = (int *)(blob.data() + L.btot), *cnt = (int *)(blob.data() + L.cnt);
    const size_t tiles = pd_ing_tiles(3000);
    for (size_t d = 0; d < PD_ING_DIGITS; ++d)
        for (size_t t = 0; t < tiles; ++t) hist[d * tiles + t] = 1;
    for (int d = 0; d < PD_ING_DIGITS; ++d) btot[d] = 2;
    for (int q = 0; q <= 65 * 65; ++q) cnt[q] = 3;
    ((int *)(blob.data() + L.src))[2999] = 4;
    printf("%zu\n", L.total);
    return 0;
}
"""


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_layout_is_ordered_aligned_disjoint_and_matches_the_documented_formula(tmp_path):
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text(_PROGRAM)
    out = subprocess.run(["hipcc", "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                          "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr[-2000:])
    assert int(run.stdout.split()[-1]) > 0
