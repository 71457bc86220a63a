// Stand-alone host test of the list passes' entries per batch (csrc/vt_plan.h: list_width,
// spec_index / spec_lane, and list_use, take_plan, take_batch at batch sizes 1, 2 and 4), the
// arithmetic vt_scan_plane_kernel<64, false, true> runs.  Four parts:
//   1. list_width over every (entries, per, fill, nqc) of the ranges below;
//   2. launches of one template block's thread blocks, simulated entry by entry as the kernel
//      walks them, the width changing from launch to launch on counters that are never reset;
//   3. the lanes that read the static batch's ids before the list's length is known;
//   4. the grid's two block numberings (block_id).
// Built with the host compiler and -fsanitize=address,undefined by tests/test_list_width.py.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <algorithm>

#include "vt_plan.h"

static int g_failed = 0;
static long g_checks = 0;
#define CHECK(c, ...)                                    \
    do {                                                 \
        ++g_checks;                                      \
        if (!(c)) {                                      \
            if (++g_failed <= 20) {                      \
                printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #c); \
                printf(__VA_ARGS__);                     \
                printf("\n");                            \
            }                                            \
        }                                                \
    } while (0)

static const int NQCS[] = {1, 2, 7, 8, 16, 32, 128};
constexpr int MAXLEN = 200, MAXBLK = 128;

// --- 1. the rule
static void check_rule() {
    for (int nqc : NQCS)
        for (int per = 1; per <= 4; ++per)
            for (int entries = 0; entries <= 2000; ++entries) {
                const int u4 = vt_plan::list_use(entries, 4, per, nqc), u2 = vt_plan::list_use(entries, 2, per, nqc),
                          u1 = vt_plan::list_use(entries, 1, per, nqc);
                CHECK(u4 >= 1 && u4 <= u2 && u2 <= u1 && u1 <= nqc, "entries %d per %d nqc %d: use %d %d %d", entries,
                      per, nqc, u4, u2, u1);
                for (int fill = 1; fill <= 512; ++fill) {
                    const int w = vt_plan::list_width(entries, per, fill, nqc);
                    bool ok = w == 4 || w == 2 || w == 1;
                    if (w == 4) ok = u4 >= fill;                           // the widest that reaches fill ...
                    if (w == 2) ok = u4 < fill && u2 >= fill;              // ... the next wider one misses it
                    if (w == 1) ok = u4 < fill && u2 < fill;               // (whether 1 reaches it or none does)
                    if (fill <= 1) ok = ok && w == 4;
                    ++g_checks;
                    if (!ok) CHECK(false, "entries %d per %d fill %d nqc %d: width %d (use %d %d %d)", entries, per,
                                   fill, nqc, w, u4, u2, u1);
                }
            }
    // the headline: 16 template blocks on 512 resident thread blocks, a grid of 128 per block
    CHECK(vt_plan::list_width(63, 1, 32, 128) == 2 && vt_plan::list_use(63, 2, 1, 128) == 32, "pass B1");
    CHECK(vt_plan::list_width(942, 4, 32, 128) == 4 && vt_plan::list_use(942, 4, 4, 128) == 64, "pass B2");
    CHECK(vt_plan::list_width(10240, 4, 32, 128) == 4, "an all-miss list");
    CHECK(vt_plan::list_width(3, 3, 1, 32) == 4, "more template blocks than resident thread blocks");
    // one resident round: 70 entries in batches of 2 are 35 batches on 32 blocks, not on 40
    CHECK(vt_plan::list_use(70, 2, 1, 128) == 40 && vt_plan::list_round(40, 32, 128) == 32, "one round");
    for (int nqc : NQCS)
        for (int use = 1; use <= nqc; ++use)
            for (int fill = 1; fill <= 512; ++fill) {
                const int r = vt_plan::list_round(use, fill, nqc);
                CHECK(r >= 1 && r <= use && (nqc < 8 || use % 8 || (r % 8 == 0 && r >= 8)) && (r == use || r >= fill),
                      "use %d fill %d nqc %d: %d", use, fill, nqc, r);
            }
}

// --- 2. the walk
struct Block {
    vt_plan::Take tk;
    int g;
};
enum Order { InOrder, Reversed, Shuffled };

// The entries of batch b of group g, as plane_wave / plane_batch index them.
static void compute(int (&done)[MAXLEN + 4], int len, int W, int G, int g, int b) {
    const int qb = (b * G + g) * W, nb = std::min(W, len - qb);
    CHECK(nb >= 1 && nb <= W, "len %d W %d: batch %d of group %d holds %d entries", len, W, b, g, nb);
    for (int e = 0; e < nb; ++e) done[qb + e]++;
}

// One launch at W entries per batch: nqc blocks per template block in the grid, the first
// list_use serve -- by the rule (fill > 0) no more than one resident round of them
// (list_round).  ctr[8] persists.  Returns the number of blocks that take.
static int launch(int len, int W, int per, int nqc, unsigned (&ctr)[8], Order order, unsigned seed, int fill = 0) {
    if (len == 0) return 0;   // every block of an empty list leaves on its length
    int use = vt_plan::list_use(len, W, per, nqc);
    if (fill > 0 && W < 4) use = vt_plan::list_round(use, fill, nqc);
    CHECK(use >= 1 && use <= nqc && use <= MAXBLK && (nqc < 8 || use % 8 == 0), "len %d W %d per %d nqc %d use %d",
          len, W, per, nqc, use);
    // (the kernel takes G and g from the grid's nqc before it knows `use`)
    CHECK(vt_plan::take_groups(use) == vt_plan::take_groups(nqc), "groups of the grid and of the serving blocks");
    const int G = vt_plan::take_groups(use);
    static int done[MAXLEN + 4];
    for (int& x : done) x = 0;
    int touched[8] = {0}, last_seen[8] = {0};
    static Block blk[MAXBLK];
    int takers[MAXBLK], ntakers = 0;
    for (int l = 0; l < use; ++l) {
        const vt_plan::Take tk = vt_plan::take_plan(len, W, l, use);
        const int g = vt_plan::take_group_of(l, use);
        CHECK(g == vt_plan::take_group_of(l, nqc), "group of block %d", l);
        CHECK(!(tk.takes && tk.sb >= tk.nbatch), "a block without a static batch takes");
        if (tk.sb < tk.nbatch) compute(done, len, W, G, g, tk.sb);
        blk[l] = {tk, g};
        if (tk.takes) takers[ntakers++] = l;
    }
    std::minstd_rand rng(seed + 1);
    const int ntakers0 = ntakers;
    if (order == Reversed) std::reverse(takers, takers + ntakers);
    long guard = 0;
    while (ntakers > 0 && ++guard < 1000000) {
        const size_t k = order == Shuffled ? rng() % ntakers : 0;
        Block& b = blk[takers[k]];
        const unsigned t = ctr[b.g]++;   // the atomic add
        touched[b.g] = 1;
        const int batch = vt_plan::take_batch(b.tk, t);
        if (batch >= 0 && batch < b.tk.nbatch) {
            compute(done, len, W, G, b.g, batch);
        } else {   // the block's one failed take
            if (t == b.tk.last) {
                last_seen[b.g]++;
                ctr[b.g] = 0u;   // the rewind
            }
            for (int i = (int)k; i + 1 < ntakers; ++i) takers[i] = takers[i + 1];   // (keeps the order)
            --ntakers;
        }
    }
    CHECK(ntakers == 0, "takes never ended");
    for (int e = 0; e < MAXLEN + 4; ++e)
        CHECK(done[e] == (e < len ? 1 : 0), "len %d W %d per %d nqc %d order %d: entry %d computed %d times", len, W,
              per, nqc, (int)order, e, done[e]);
    for (int g = 0; g < 8; ++g) {
        CHECK(last_seen[g] == touched[g], "len %d W %d per %d nqc %d order %d: group %d touched %d, last users %d",
              len, W, per, nqc, (int)order, g, touched[g], last_seen[g]);
        CHECK(ctr[g] == 0u, "len %d W %d per %d nqc %d order %d: counter %d left at %u", len, W, per, nqc, (int)order,
              g, ctr[g]);   // (left as it is: the next launch starts from it)
    }
    return ntakers0;
}

static void check_walk() {
    static const int widths[] = {4, 1, 2, 2, 4, 1};
    unsigned ctr[8] = {0};
    unsigned seed = 1;
    size_t wi = 0;
    for (int len = 0; len <= MAXLEN; ++len)
        for (int per = 1; per <= 4; ++per)
            for (int nqc : NQCS) {
                const int other = (len * 7 + 13) % (MAXLEN + 1);   // another list on the same counters
                int takers = 0;
                for (int W : {1, 2, 4}) {
                    takers = std::max(takers, launch(len, W, per, nqc, ctr, InOrder, 0));
                    launch(other, widths[wi++ % 6], per, nqc, ctr, InOrder, 0);
                    launch(len, W, per, nqc, ctr, Reversed, 0);
                }
                // the rule's own width, for a few values of fill
                for (int fill : {1, 3, 8, 30, 32, 170, 512}) {
                    const int W = vt_plan::list_width(len, per, fill, nqc);
                    launch(len, W, per, nqc, ctr, Reversed, 0, fill);
                    for (int s = 0; s < 4; ++s) launch(len, W, per, nqc, ctr, Shuffled, seed++, fill);
                }
                // (with fewer than two taking blocks at every width every order is the same one)
                const int nshuf = takers >= 2 ? 300 : 3;
                for (int s = 0; s < nshuf; ++s) {
                    launch(len, widths[wi++ % 6], per, nqc, ctr, Shuffled, seed++);
                    if (s % 50 == 0) launch(other, widths[wi++ % 6], per, nqc, ctr, Shuffled, seed++);
                }
            }
}

// --- 3. the speculative id lanes: for every width the length may choose, lanes
// spec_lane(W) .. + W - 1 hold exactly the static batch's entries, and no lane's index leaves
// the slab (ld entries: the call's queries, at least the list's length)
static void check_spec() {
    for (int W : {1, 2, 4}) {
        const int base = vt_plan::spec_lane(W);
        CHECK(base >= 0 && base + W <= 8, "lanes of width %d", W);
        for (int e = 0; e < W; ++e)
            CHECK(vt_plan::spec_width(base + e) == W && vt_plan::spec_entry(base + e) == e, "lane %d", base + e);
    }
    {   // the three widths' lanes are disjoint: 4 + 2 + 1 of every eight
        int seen[8] = {0};
        for (int W : {1, 2, 4})
            for (int e = 0; e < W; ++e) seen[vt_plan::spec_lane(W) + e]++;
        for (int i = 0; i < 7; ++i) CHECK(seen[i] == 1, "lane %d serves %d widths", i, seen[i]);
    }
    for (int nqc : NQCS)
        for (int per = 1; per <= 4; ++per)
            for (int len = 1; len <= MAXLEN; ++len)
                for (int ld : {len, len + 1, 300, 10240}) {
                    const int G = vt_plan::take_groups(nqc);
                    for (int l = 0; l < nqc; ++l) {   // every block of the grid reads before it knows
                        const int g = vt_plan::take_group_of(l, nqc), sbg = (G == 8 ? l >> 3 : l) * G + g;
                        for (int lane = 0; per == 1 && lane < 64; ++lane) {   // (no function of per)
                            const int i = vt_plan::spec_index(sbg, lane, ld);
                            CHECK(i >= 0 && i < ld, "nqc %d l %d lane %d ld %d: index %d", nqc, l, lane, ld, i);
                        }
                        for (int W : {1, 2, 4}) {
                            const int use = vt_plan::list_use(len, W, per, nqc);
                            if (l >= use) continue;
                            const vt_plan::Take tk = vt_plan::take_plan(len, W, l, use);
                            if (tk.sb >= tk.nbatch) continue;   // no static batch: the block leaves
                            const int qb = (tk.sb * G + g) * W, nb = std::min(W, len - qb);
                            CHECK(nb >= 1, "static batch");
                            for (int e = 0; e < nb; ++e)
                                CHECK(vt_plan::spec_index(sbg, vt_plan::spec_lane(W) + e, ld) == qb + e,
                                      "len %d ld %d W %d per %d nqc %d l %d: entry %d read at %d, is %d", len, ld, W,
                                      per, nqc, l, e, vt_plan::spec_index(sbg, vt_plan::spec_lane(W) + e, ld), qb + e);
                        }
                    }
                }
}

// --- 4. the two numberings of the grid's blocks: each (template block, block of it) once
static void check_block_ids() {
    static int seen[40 * 128];
    for (int ntb : {1, 2, 3, 16, 17, 40})
        for (int nqc : NQCS)
            for (int lfirst = 0; lfirst < 2; ++lfirst) {
                for (int i = 0; i < ntb * nqc; ++i) seen[i] = 0;
                for (int b = 0; b < ntb * nqc; ++b) {
                    const vt_plan::BlockId id = vt_plan::block_id((unsigned)b, ntb, nqc, lfirst != 0);
                    const bool in = id.tb >= 0 && id.tb < ntb && id.l >= 0 && id.l < nqc;
                    CHECK(in, "ntb %d nqc %d lfirst %d block %d: (%d, %d)", ntb, nqc, lfirst, b, id.tb, id.l);
                    if (in) seen[id.tb * nqc + id.l]++;
                    if (lfirst && b + 1 < ntb * nqc)   // the l-th blocks of all template blocks side by side
                        CHECK(id.l == b / ntb, "block %d", b);
                }
                for (int i = 0; i < ntb * nqc; ++i) CHECK(seen[i] == 1, "ntb %d nqc %d lfirst %d", ntb, nqc, lfirst);
            }
}

int main() {
    check_block_ids();
    check_rule();
    check_walk();
    check_spec();
    printf("%ld checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
