// Stand-alone host test of the plane scan's batch assignment (csrc/vt_plan.h: list_use,
// take_plan, take_batch), the arithmetic the kernel runs: launches of one template block's
// thread blocks are simulated with the individual counter takes interleaved in many orders,
// on counters that are never reset between launches (as the library's are not).  Built with
// the host compiler and -fsanitize=address,undefined by tests/test_list_take.py.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <algorithm>

#include "vt_plan.h"

static int g_failed = 0, g_checks = 0;
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

constexpr int NB = 4;   // queries per batch (the kernel's PL_NB)
constexpr int MAXB = 64, MAXBLK = 128;   // batches of the longest list, blocks of the widest grid

struct Block {
    vt_plan::Take tk;
    int g;
    bool done;
};

enum Order { InOrder, Reversed, RoundRobin, Shuffled };

// One launch: `nblk_grid` blocks per template block; list: the first list_use serve; dense
// (per == 0): all do.  ctr[8] persists.  Returns the number of blocks that take.
static int launch(int len, int per, int nqc, unsigned (&ctr)[8], Order order, unsigned seed) {
    if (len == 0) return 0;   // every block of an empty list leaves on its length
    const int use = per ? vt_plan::list_use(len, NB, per, nqc) : nqc;
    CHECK(use >= 1 && use <= nqc && (nqc < 8 || use % 8 == 0), "len %d per %d nqc %d use %d", len, per, nqc, use);
    const int G = vt_plan::take_groups(use), nbt = (len + NB - 1) / NB;
    static int done[8][MAXB + 1];   // [group][batch of the group]
    CHECK(nbt <= MAXB && use <= MAXBLK, "sizes");
    for (auto& row : done)
        for (int& x : row) x = 0;
    int touched[8] = {0}, last_seen[8] = {0}, nbatch_g[8] = {0};
    for (int B = 0; B < nbt; ++B) nbatch_g[B % G]++;   // batch B belongs to group B % G (independent count)
    static Block blk[MAXBLK];
    int takers[MAXBLK], ntakers = 0;
    for (int l = 0; l < use; ++l) {
        const vt_plan::Take tk = vt_plan::take_plan(len, NB, l, use);
        const int g = vt_plan::take_group_of(l, use);
        CHECK(g >= 0 && g < G, "group");
        CHECK(tk.nbatch == nbatch_g[g], "len %d use %d l %d: nbatch %d vs %d", len, use, l, tk.nbatch, nbatch_g[g]);
        CHECK(!(tk.takes && tk.sb >= tk.nbatch), "a block without a static batch takes");
        if (tk.sb < tk.nbatch) done[g][tk.sb]++;
        blk[l] = {tk, g, !tk.takes};
        if (tk.takes) takers[ntakers++] = l;
    }
    std::minstd_rand rng(seed + 1);
    const int ntakers0 = ntakers;
    if (order == Reversed) std::reverse(takers, takers + ntakers);
    size_t rr = 0;
    long guard = 0;
    while (ntakers > 0 && ++guard < 1000000) {
        const size_t k = order == Shuffled ? rng() % ntakers : order == RoundRobin ? rr++ % ntakers : 0;
        Block& b = blk[takers[k]];
        const unsigned t = ctr[b.g]++;   // the atomic add
        touched[b.g] = 1;
        const int batch = vt_plan::take_batch(b.tk, t);
        if (batch >= 0 && batch < b.tk.nbatch) {
            done[b.g][batch]++;
        } else {   // the block's one failed take
            b.done = true;
            if (t == b.tk.last) {
                last_seen[b.g]++;
                ctr[b.g] = 0u;   // the rewind
            }
            for (int i = (int)k; i + 1 < ntakers; ++i) takers[i] = takers[i + 1];   // (keeps the order)
            --ntakers;
        }
    }
    CHECK(ntakers == 0, "takes never ended");
    for (int g = 0; g < 8; ++g) {
        for (int b = 0; b < (g < G ? nbatch_g[g] : 0); ++b)
            CHECK(done[g][b] == 1, "len %d per %d nqc %d order %d: batch %d of group %d computed %d times", len, per,
                  nqc, (int)order, b, g, done[g][b]);
        CHECK(last_seen[g] == touched[g], "len %d per %d nqc %d order %d: group %d touched %d, last users %d", len,
              per, nqc, (int)order, g, touched[g], last_seen[g]);
        CHECK(ctr[g] == 0u, "len %d per %d nqc %d order %d: counter %d left at %u", len, per, nqc, (int)order, g,
              ctr[g]);   // (left as it is: the next launch starts from it)
    }
    return ntakers0;
}

int main() {
    static const int nqcs[] = {1, 2, 7, 8, 16, 32, 128};
    unsigned ctr[8] = {0};
    unsigned seed = 1;
    for (int len = 0; len <= 200; ++len)
        for (int per = 1; per <= 4; ++per)
            for (int nqc : nqcs) {
                const int other = (len * 7 + 13) % 201;   // a second launch of another length on the same counters
                launch(len, per, nqc, ctr, InOrder, 0);
                launch(other, per, nqc, ctr, InOrder, 0);
                launch(len, per, nqc, ctr, Reversed, 0);
                launch(other, per == 1 ? 3 : 1, nqc, ctr, Reversed, 0);
                // (with fewer than two taking blocks every order is the same one)
                const int nshuf = launch(len, per, nqc, ctr, RoundRobin, 0) >= 2 ? 300 : 2;
                for (int s = 0; s < nshuf; ++s) {
                    launch(len, per, nqc, ctr, Shuffled, seed++);
                    if (s % 50 == 0) launch(other, per, nqc, ctr, Shuffled, seed++);
                }
                if (per == 1) {   // the dense launch: every block of the grid serves
                    launch(len, 0, nqc, ctr, InOrder, 0);
                    launch(len, 0, nqc, ctr, Reversed, 0);
                    for (int s = 0; s < 20; ++s) launch(len, 0, nqc, ctr, Shuffled, seed++);
                }
            }
    // pass B2's batches per block: 4 below the resident thread blocks, 3 from there on
    CHECK(vt_plan::list_per(16, 512) == 4 && vt_plan::list_per(157, 512) == 4, "few template blocks");
    CHECK(vt_plan::list_per(512, 512) == 3 && vt_plan::list_per(1563, 512) == 3, "many template blocks");
    printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
