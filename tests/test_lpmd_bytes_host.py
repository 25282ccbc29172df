"""The byte form of the LPMD windowed pair count (metheor_amd/csrc/mth_lpmd_bytes.h) compiled as plain C++ and compared, read by
read, with the naive double loop (readutil.rs:166-224: min <= rel_k - rel_j <= max, discordant = the two states differ).
No GPU: the header's stand-ins replace v_alignbyte / v_perm / v_bitop3 and the wave vote (one lane)."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "metheor_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "mth_lpmd_bytes.h"
using namespace mth;

static uint64_t rs = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (uint32_t)(rs >> 16); }

static LpMask M[9][8];
static long n_cases = 0, n_pairs_in = 0, n_far = 0;

// rel[0..n): ascending; st[0..n): 0 / 1.  Everything else about the 8 slots is random.
static int check(const int n, const int *rel, const int *st, const int mind, const int maxd) {
    uint32_t E[2] = {rnd(), rnd()}, v[8];
    for (int k = 0; k < 8; ++k) v[k] = rnd();                       // dead slots: any word; live ones: position bits and 7 junk state-byte bits
    for (int k = 0; k < n; ++k) {
        E[k >> 2] = (E[k >> 2] & ~(0xffu << (8 * (k & 3)))) | ((uint32_t)rel[k] << (8 * (k & 3)));
        v[k] = (v[k] & 0x7fffffffu) | ((uint32_t)st[k] << 31);
    }
    uint32_t want_c = 0, want_d = 0;
    for (int k = 1; k < n; ++k)
        for (int j = 0; j < k; ++j) {
            const int d = rel[k] - rel[j];
            if (d > 127) n_far += 1;
            if (d < mind || d > maxd) continue;
            if (st[k] == st[j]) want_c += 1; else want_d += 1;
        }
    uint32_t got_c = 1000, got_d = 7;                                // the helper ADDS
    lpmd_pairs_bytes(E[0], E[1], lpmd_state_bytes(v[0], v[1], v[2], v[3]), lpmd_state_bytes(v[4], v[5], v[6], v[7]), &M[n][0],
                     (uint32_t)mind, (uint32_t)maxd, got_c, got_d);
    n_cases += 1; n_pairs_in += want_c + want_d;
    if (got_c != 1000 + want_c || got_d != 7 + want_d) {
        printf("MISMATCH n=%d min=%d max=%d got %u/%u want %u/%u rel:", n, mind, maxd, got_c - 1000, got_d - 7, want_c, want_d);
        for (int k = 0; k < n; ++k) printf(" %d%c", rel[k], st[k] ? 'Z' : 'z');
        printf("\n");
        return 1;
    }
    return 0;
}

int main() {
    for (uint32_t n = 0; n < 9; ++n)
        for (uint32_t g = 0; g < 8; ++g) { M[n][g].w0 = lpmd_bytes_mask(n, g, 0); M[n][g].w1 = lpmd_bytes_mask(n, g, 1); }
    const int mins[] = {0, 1, 2, 127, 128}, maxs[] = {0, 1, 16, 126, 127};
    const int steps[] = {0, 1, 2, 15, 16, 17, 126, 127, 128, 129, 254, 255};     // gaps between adjacent calls worth hitting exactly
    int bad = 0;
    for (int mi = 0; mi < 5; ++mi)
        for (int ma = 0; ma < 5; ++ma) {
            const int mind = mins[mi], maxd = maxs[ma];
            if (!lpmd_bytes_domain(mind, maxd)) { printf("DOMAIN %d %d\n", mind, maxd); return 2; }
            for (int n = 0; n <= 8; ++n) {
                int rel[8], st[8];
                // hand-picked shapes: all equal; one gap of an exact size at every place, the rest equal or adjacent
                for (int si = 0; si < 12; ++si)
                    for (int at = 0; at < (n > 1 ? n - 1 : 1); ++at)
                        for (int fill = 0; fill < 2; ++fill)
                            for (int base = 0; base < 2; ++base) {
                                int x = base ? 255 : 0, ok = 1;
                                for (int k = 0; k < n; ++k) {
                                    if (k) x += (k - 1 == at) ? steps[si] : fill;
                                    rel[k] = x; st[k] = (int)(rnd() & 1u);
                                }
                                if (base) { const int sh = n ? rel[n - 1] - 255 : 0; for (int k = 0; k < n; ++k) { rel[k] -= sh; if (rel[k] < 0) ok = 0; } }   // last call at 255
                                if (n && rel[n - 1] > 255) ok = 0;
                                if (ok) bad += check(n, rel, st, mind, maxd);
                            }
                // random ascending reads: dense, medium and sparse spacing
                for (int it = 0; it < 3000; ++it) {
                    const int spread = (it % 3 == 0) ? 4 : (it % 3 == 1 ? 40 : 256);
                    int x = (int)(rnd() % 256u), ok = 1;
                    for (int k = 0; k < n; ++k) {
                        if (k) x += (int)(rnd() % (uint32_t)spread);
                        if (x > 255) { if (it & 1) x = 255; else ok = 0; }
                        rel[k] = x; st[k] = (int)(rnd() & 1u);
                    }
                    if (ok) bad += check(n, rel, st, mind, maxd);
                }
                if (bad > 20) return 1;
            }
        }
    // distances of exactly 127, 128, 254 and 255 between the first and the last call, in every window
    {
        const int ds[] = {127, 128, 254, 255};
        for (int di = 0; di < 4; ++di)
            for (int n = 2; n <= 8; ++n)
                for (int mi = 0; mi < 5; ++mi)
                    for (int ma = 0; ma < 5; ++ma) {
                        int rel[8], st[8];
                        for (int k = 0; k < n; ++k) { rel[k] = (k == n - 1) ? ds[di] : 0; st[k] = k & 1; }
                        bad += check(n, rel, st, mins[mi], maxs[ma]);
                        for (int k = 0; k < n; ++k) rel[k] = (k == 0) ? 255 - ds[di] : 255;
                        bad += check(n, rel, st, mins[mi], maxs[ma]);
                    }
    }
    printf("cases %ld pairs_in_window %ld pairs_beyond_127 %ld bad %d\n", n_cases, n_pairs_in, n_far, bad);
    return bad ? 1 : 0;
}
"""


def test_byte_form_matches_naive_loop(tmp_path):
    src = tmp_path / "lpmd_bytes_driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "lpmd_bytes_driver"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-I", CSRC, "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1].split()
    # not vacuous: many reads, pairs inside the window, and pairs farther apart than a byte's sign bit
    assert int(last[1]) > 500_000 and int(last[3]) > 100_000 and int(last[5]) > 100_000 and int(last[7]) == 0

