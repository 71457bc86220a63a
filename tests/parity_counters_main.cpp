// The single list pass's counters by call parity (csrc/vt_plan.h: ParityCounters, parity_grows,
// parity_grown, parity_begin, parity_last_offset), driven as vt_launch_pruned drives them, on
// the host: a buffer that is zeroed only when it is (re)allocated, calls of varying template-block
// counts and list lengths, each of which zeroes the nzero counters of the other parity, then
// appends to its own.  Checked: every call finds every counter it may append to at zero; the
// call's counts are readable (parity_last_offset) until the next call begins, through any
// number of reads; the offsets stay inside the buffer.  Allocations are exact (2 * cap words,
// filled with a poison at malloc and zeroed as the host zeroes them), so AddressSanitizer sees
// any index past them.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vt_plan.h"

namespace {

int failed = 0, checks = 0;
void check(bool ok, const char* what, int call) {
    ++checks;
    if (!ok) {
        ++failed;
        std::printf("FAILED call %d: %s\n", call, what);
    }
}

struct Sim {
    vt_plan::ParityCounters s;
    unsigned* buf = nullptr;   // [2][cap], exact
    std::vector<unsigned> last;   // the last call's counts, as the lists were filled
    ~Sim() { std::free(buf); }

    // One pruned call over ntb template blocks; list tb gets len(tb) entries.
    template <class Len>
    void call(int ntb, Len&& len, int n) {
        if (vt_plan::parity_grows(s, ntb)) {
            vt_plan::ParityCounters g = s;
            vt_plan::parity_grown(g, ntb);
            check(g.cap >= ntb, "grown capacity", n);
            std::free(buf);
            buf = static_cast<unsigned*>(std::malloc(sizeof(unsigned) * 2 * (size_t)g.cap));
            for (size_t i = 0; i < 2 * (size_t)g.cap; ++i) buf[i] = 0u;   // the allocation's memset
            g.par = 0;
            s = g;
        }
        const vt_plan::ParityCall c = vt_plan::parity_begin(s, ntb);
        check(c.mine + (size_t)ntb <= 2 * (size_t)s.cap && c.other + (size_t)c.nzero <= 2 * (size_t)s.cap,
              "offsets inside the buffer", n);
        check(c.mine != c.other && (c.mine == 0 || c.other == 0), "two parities", n);
        // the front kernel's first thread block: the other parity's counters back to zero
        for (int b = 0; b < c.nzero; ++b) buf[c.other + b] = 0u;
        // every counter this call may append to starts from zero (all of its parity: a later
        // call with more template blocks must find them zero too)
        bool zero = true;
        for (int b = 0; b < s.cap; ++b) zero = zero && buf[c.mine + b] == 0u;
        check(zero, "the call's counters start from zero", n);
        last.assign((size_t)ntb, 0u);
        for (int tb = 0; tb < ntb; ++tb) {
            const unsigned entries = len(tb);
            for (unsigned e = 0; e < entries; ++e) last[(size_t)tb] = ++buf[c.mine + tb];   // the appends
        }
    }
    // rs_vt_prune_scanned: the last call's counts
    void read(int n) {
        check(s.last >= 0, "a last call", n);
        const size_t off = vt_plan::parity_last_offset(s);
        bool same = true;
        for (size_t tb = 0; tb < last.size(); ++tb) same = same && buf[off + tb] == last[tb];
        check(same, "the last call's counts are readable", n);
    }
};

}  // namespace

int main() {
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() {
        rng ^= rng << 13;
        rng ^= rng >> 7;
        rng ^= rng << 17;
        return (unsigned)(rng >> 33);
    };
    const int shapes[] = {1, 3, 17, 2, 16, 5, 40, 39, 1, 157, 3, 156, 400, 17};
    for (int trial = 0; trial < 40; ++trial) {
        Sim sim;
        int n = 0;
        for (int rep = 0; rep < 6; ++rep)
            for (const int shape : shapes) {
                // the same library for a few calls, then another (a grown library, a shard)
                const int ntb = trial < 8 ? shape : 1 + (int)(next() % 300u);
                const int calls = 1 + (int)(next() % 4u);
                for (int k = 0; k < calls; ++k, ++n) {
                    const unsigned mode = next() % 4u;   // all empty, all full, mixed, one block only
                    const unsigned nq = 1u + next() % 50u;
                    const unsigned only = next() % (unsigned)ntb;
                    sim.call(ntb, [&](int tb) {
                        return mode == 0 ? 0u : mode == 1 ? nq : mode == 2 ? next() % (nq + 1u) : ((unsigned)tb == only ? nq : 0u);
                    }, n);
                    const int reads = (int)(next() % 3u);   // none, once, twice
                    for (int r = 0; r < reads; ++r) sim.read(n);
                }
            }
    }
    // the single list's fill (vt_plan::single_pass_fill): four rounds' worth, inside the kernel
    // argument's 16 bits; at the headline (fill 32, per 4, 128 blocks per template block) lists of
    // about a thousand entries take batches of 2 and all-miss lists keep 4
    for (int fill = 0; fill <= 70000; fill += fill < 600 ? 1 : 997) {
        const int f = vt_plan::single_pass_fill(fill);
        check(f >= 1 && f <= 65535 && (f == 65535 || f == 4 * (fill < 1 ? 1 : fill)), "single_pass_fill", fill);
    }
    check(vt_plan::list_width(1005, 4, vt_plan::single_pass_fill(32), 128) == 2, "headline lists: 2 per batch", 0);
    check(vt_plan::list_width(942, 4, 32, 128) == 4, "pass B2 keeps 4 at the headline", 0);
    check(vt_plan::list_width(10240, 4, vt_plan::single_pass_fill(32), 128) == 4, "all-miss lists keep 4", 0);
    std::printf("%d checks, %d failed\n", checks, failed);
    return failed ? 1 : 0;
}
