"""The diagonal walk of the byte-form LPMD pair count (metheor_amd/csrc/mth_lpmd_bytes.h) compiled as plain C++: where it stops and
that the counts do not depend on it.  One lane is its own vote there, so the stop rule -- go on to diagonal g + 1 only if two ADJACENT
pairs of diagonal g lie within max_distance -- is exercised read by read against a model of the rule, and the counts against the naive
double loop (readutil.rs:166-224).  Also: the live-byte mask LB(n) and its shifts against lpmd_bytes_mask for every (n, g, word).
No GPU."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "metheor_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "mth_lpmd_bytes.h"
using namespace mth;

static uint64_t rs = 0x2545f4914f6cdd1dull;
static uint32_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (uint32_t)(rs >> 16); }

static LpMask M[9][8];
static long n_cases = 0, n_pairs_in = 0, n_early = 0, n_waste = 0, walked_hist[8];

// the rule, one lane: diagonal g is evaluated; g + 1 follows iff some j has (j, j + g) and (j + 1, j + g + 1) both live and within max
static int model_walk(const int n, const int *rel, const int maxd) {
    int g = 1;
    for (; g < 7; ++g) {
        bool adj = false;
        for (int j = 0; j + g + 1 < n; ++j) adj |= rel[j + g] - rel[j] <= maxd && rel[j + g + 1] - rel[j + 1] <= maxd;
        if (!adj) break;
    }
    return g;
}
// the last diagonal that holds a pair within max (0: none): what an exact walk would need
static int need_walk(const int n, const int *rel, const int maxd) {
    int last = 0;
    for (int g = 1; g < 8; ++g)
        for (int j = 0; j + g < n; ++j) if (rel[j + g] - rel[j] <= maxd) last = g;
    return last;
}

// rel[0..n): ascending; st[0..n): 0 / 1.  dead: bytes for the dead slots (nullptr: random); everything else about the 8 slots is random.
// want_walk >= 0: the number of diagonals this read must make the walk evaluate.
static int check(const int n, const int *rel, const int *st, const int mind, const int maxd, const int *dead = nullptr, const int want_walk = -1) {
    uint32_t E[2] = {rnd(), rnd()}, v[8];
    for (int k = 0; k < 8; ++k) v[k] = rnd();                       // dead slots: any word; live ones: position bits and 7 junk state-byte bits
    for (int k = 0; k < 8; ++k) {
        if (k >= n && !dead) continue;
        const uint32_t b = (uint32_t)(k < n ? rel[k] : dead[k]) & 0xffu;
        E[k >> 2] = (E[k >> 2] & ~(0xffu << (8 * (k & 3)))) | (b << (8 * (k & 3)));
    }
    for (int k = 0; k < n; ++k) v[k] = (v[k] & 0x7fffffffu) | ((uint32_t)st[k] << 31);
    uint32_t want_c = 0, want_d = 0;
    for (int k = 1; k < n; ++k)
        for (int j = 0; j < k; ++j) {
            const int d = rel[k] - rel[j];
            if (d < mind || d > maxd) continue;
            if (st[k] == st[j]) want_c += 1; else want_d += 1;
        }
    const LpMask lb = lpmd_live_bytes((uint32_t)n);
    uint32_t got_c = 1000, got_d = 7, walked = 0;                    // the helper ADDS
    lpmd_pairs_bytes(E[0], E[1], lpmd_state_bytes(v[0], v[1], v[2], v[3]), lpmd_state_bytes(v[4], v[5], v[6], v[7]), lb.w0, lb.w1,
                     (uint32_t)mind, (uint32_t)maxd, got_c, got_d, &walked);
    {   // the table form (masks read from the row M[n][.]) gives the same counts and the same walk
        uint32_t tc = 1000, td = 7, tw = 0;
        lpmd_pairs_bytes(E[0], E[1], lpmd_state_bytes(v[0], v[1], v[2], v[3]), lpmd_state_bytes(v[4], v[5], v[6], v[7]), &M[n][0],
                         (uint32_t)mind, (uint32_t)maxd, tc, td, &tw);
        if (tc != got_c || td != got_d || tw != walked) { printf("TABLE FORM differs: %u/%u walk %u against %u/%u walk %u\n", tc, td, tw, got_c, got_d, walked); return 1; }
    }
    const int model = model_walk(n, rel, maxd), need = need_walk(n, rel, maxd);
    n_cases += 1; n_pairs_in += want_c + want_d;
    n_early += model < 7 ? 1 : 0; n_waste += model - (need > 1 ? need : 1);
    walked_hist[model] += 1;
    int bad = 0;
    if (got_c != 1000 + want_c || got_d != 7 + want_d) { printf("MISMATCH counts got %u/%u want %u/%u", got_c - 1000, got_d - 7, want_c, want_d); bad = 1; }
    else if ((int)walked != model) { printf("MISMATCH walk %u, the rule says %d", walked, model); bad = 1; }
    else if (model < need) { printf("MODEL stops at %d before a pair on %d", model, need); bad = 1; }      // the rule itself would lose a pair
    else if (want_walk >= 0 && (int)walked != want_walk) { printf("MISMATCH walk %u, the case was built for %d", walked, want_walk); bad = 1; }
    if (bad) {
        printf(" n=%d min=%d max=%d rel:", n, mind, maxd);
        for (int k = 0; k < n; ++k) printf(" %d%c", rel[k], st[k] ? 'Z' : 'z');
        printf("\n");
    }
    return bad;
}

int main() {
    int bad = 0;
    for (uint32_t n = 0; n < 9; ++n)
        for (uint32_t g = 0; g < 8; ++g) { M[n][g].w0 = lpmd_bytes_mask(n, g, 0); M[n][g].w1 = lpmd_bytes_mask(n, g, 1); }
    // LB(n) and its shifts are the rows of the table they replace (n beyond 8: the row of 8)
    for (uint32_t n = 0; n <= 20; ++n) {
        const LpMask lb = lpmd_live_bytes(n);
        for (uint32_t g = 0; g < 8; ++g)
            for (uint32_t w = 0; w < 2; ++w) {
                const uint32_t want = lpmd_bytes_mask(n < 8 ? n : 8, g, w);
                const uint32_t got = w ? lpmd_mask_w1(lb.w0, lb.w1, (int)g) : lpmd_mask_w0(lb.w0, lb.w1, (int)g);
                if (got != want) { printf("MASK n=%u g=%u w=%u got %08x want %08x\n", n, g, w, got, want); bad += 1; }
            }
    }
    if (bad) return 1;
    const int mins[] = {0, 1, 2, 127, 128}, maxs[] = {0, 1, 16, 126, 127};
    for (int mi = 0; mi < 5; ++mi)
        for (int ma = 0; ma < 5; ++ma) {
            const int mind = mins[mi], maxd = maxs[ma];
            if (!lpmd_bytes_domain(mind, maxd)) { printf("DOMAIN %d %d\n", mind, maxd); return 2; }
            for (int n = 0; n <= 8; ++n) {
                int rel[8], st[8], dead[8];
                // all calls on one position (equal adjacent positions: every distance 0), at either end of the byte
                for (int base = 0; base < 256; base += 255) {
                    for (int k = 0; k < 8; ++k) { rel[k] = base; st[k] = (int)(rnd() & 1u); dead[k] = base; }
                    bad += check(n, rel, st, mind, maxd, dead, n >= 2 ? (n - 1 < 7 ? n - 1 : 7) : 1);
                }
                // random ascending reads around the window: steps of 0 .. about max, so that the walk ends on every diagonal
                for (int it = 0; it < 2500; ++it) {
                    const int spread = (it % 4 == 0) ? 2 : (it % 4 == 1 ? maxd / 2 + 2 : (it % 4 == 2 ? maxd + 3 : 256));
                    int x = (int)(rnd() % 200u), ok = 1;
                    for (int k = 0; k < n; ++k) {
                        if (k) x += (int)(rnd() % (uint32_t)spread);
                        if (x > 255) { if (it & 1) x = 255; else ok = 0; }
                        rel[k] = x; st[k] = (int)(rnd() & 1u);
                    }
                    // dead slots: random, or the last call's byte going on in steps of one (junk that looks like near calls)
                    for (int k = 0; k < 8; ++k) dead[k] = (n ? rel[n - 1] : 0) + (k - n + 1);
                    if (ok) bad += check(n, rel, st, mind, maxd, (it & 2) ? dead : nullptr);
                }
                if (bad > 20) return 1;
            }
            if (maxd < 1 || maxd > 32) continue;
            // ---- reads built on the rule's edges (windows whose max leaves room in a byte: 1 and 16)
            for (int g = 1; g <= 6; ++g)
                for (int j = 0; j + g < 8; ++j) {
                    int rel[8], st[8], dead[8];
                    for (int k = 0; k < 8; ++k) { st[k] = (int)(rnd() & 1u); dead[k] = 0; }
                    // (a) ONE pair within max on diagonal g: the cluster j .. j + g spans exactly max (its inner calls one step in), every
                    // call outside it lies max + 1 or more from its neighbours.  No two adjacent pairs on g: the walk must end there.
                    // n = 8 and n = j + g + 1 (nothing live behind the cluster; the dead bytes go on in steps of one)
                    for (int tail = 0; tail < 2; ++tail) {
                        const int n = tail ? 8 : j + g + 1;
                        for (int k = 0; k < n; ++k) {
                            if (k <= j) rel[k] = k * (maxd + 1);
                            else if (k < j + g) rel[k] = rel[j] + 1;
                            else if (k == j + g) rel[k] = rel[j] + maxd;
                            else rel[k] = rel[k - 1] + maxd + 1;
                        }
                        for (int k = n; k < 8; ++k) dead[k] = rel[n - 1] + (k - n + 1);
                        bad += check(n, rel, st, mind, maxd, dead, g);
                    }
                    // (b) two adjacent pairs on g, (j, j + g) and (j + 1, j + g + 1), and the pair they announce, (j, j + g + 1), at exactly max
                    // (over = 0: counted on diagonal g + 1) and at max + 1 (over = 1: the walk takes g + 1 and finds nothing there)
                    if (j + g + 1 < 8 && maxd >= 8)
                        for (int over = 0; over < 2; ++over) {
                            const int n = j + g + 2;
                            for (int k = 0; k < n; ++k) {
                                if (k <= j) rel[k] = k * (maxd + 1);
                                else if (k < j + g) rel[k] = rel[j] + 1;
                                else if (k == j + g) rel[k] = rel[j] + maxd - 1 + over;
                                else rel[k] = rel[j] + maxd + over;
                            }
                            for (int k = n; k < 8; ++k) dead[k] = rel[n - 1];
                            if (rel[j + g + 1] - rel[j] != maxd + over || rel[j + g] - rel[j] > maxd || rel[j + g + 1] - rel[j + 1] > maxd) { printf("CASE b g=%d j=%d\n", g, j); return 2; }
                            if (need_walk(n, rel, maxd) != g + 1 - over) { printf("CASE b need g=%d j=%d\n", g, j); return 2; }
                            bad += check(n, rel, st, mind, maxd, dead, g + 1 < 7 ? g + 1 : 7);
                        }
                }
            // (c) adjacency across the two words: the pairs (3, 3 + g) and (4, 4 + g).  Live: n = 5 + g, the walk goes on.  Not live: n = 4 + g
            // with the dead slot 4 + g holding a byte that looks like a near call -- the pair of slot 4 is masked and must not count as adjacent
            for (int g = 1; g <= 3; ++g)
                for (int live = 0; live < 2; ++live) {
                    const int n = 4 + g + live;
                    int rel[8], st[8], dead[8];
                    for (int k = 0; k < 8; ++k) { st[k] = (int)(rnd() & 1u); dead[k] = 0; }
                    for (int k = 0; k < n; ++k) rel[k] = k < 3 ? k * (maxd + 1) : 3 * (maxd + 1);      // slots 3 .. n - 1 on one position
                    for (int k = n; k < 8; ++k) dead[k] = rel[n - 1];
                    // slots 3 .. n - 1 are n - 3 calls on one position: pairs up to diagonal n - 4, adjacent ones up to n - 5
                    bad += check(n, rel, st, mind, maxd, dead, n - 4 < 7 ? n - 4 : 7);
                    // only (3, 3 + g) and, when live, (4, 4 + g) within max on diagonal g: slots 4 .. 3 + g one step on
                    if (maxd >= 2) {
                        for (int k = 4; k < n; ++k) rel[k] = rel[3] + 1;
                        for (int k = n; k < 8; ++k) dead[k] = rel[n - 1];
                        bad += check(n, rel, st, mind, maxd, dead);
                    }
                }
            // (d) eight calls two apart: every pair within 16, all seven diagonals run; one apart for max = 1: diagonal 1 only has pairs,
            // and they are adjacent, so the walk takes diagonal 2 as well
            {
                int rel[8], st[8];
                for (int k = 0; k < 8; ++k) { rel[k] = 100 + (maxd >= 14 ? 2 : 1) * k; st[k] = k & 1; }
                bad += check(8, rel, st, mind, maxd, nullptr, maxd >= 14 ? 7 : 2);
            }
        }
    long early = 0;
    for (int g = 1; g < 7; ++g) { early += walked_hist[g]; if (!walked_hist[g]) { printf("NO READ ended the walk on diagonal %d\n", g); bad += 1; } }
    if (!walked_hist[7]) { printf("NO READ ran all seven diagonals\n"); bad += 1; }
    printf("cases %ld pairs_in_window %ld ended_early %ld wasted_diagonals %ld bad %d\n", n_cases, n_pairs_in, early, n_waste, bad);
    return bad ? 1 : 0;
}
"""


def test_walk_stops_by_adjacent_pairs_and_counts_do_not_change(tmp_path):
    src = tmp_path / "lpmd_exit_driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "lpmd_exit_driver"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-I", CSRC, "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1].split()
    # not vacuous: many reads, pairs inside the window, walks that ended before the seventh diagonal
    assert int(last[1]) > 400_000 and int(last[3]) > 100_000 and int(last[5]) > 100_000 and int(last[9]) == 0
