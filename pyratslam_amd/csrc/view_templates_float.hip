// Device-resident float view-template library (rs_vtf): ViewTemplate.match on
// float32 / float64 arrays (view_templates.py:16-28) against templates kept in HBM,
// bit-exact to numpy's arithmetic.
//
// The sum of |T - Q| over the (H-2M) x W window is numpy's pairwise summation of the
// flattened n = (H-2M)*W elements.  SadPlan lowers that recursion once per handle:
//   * leaves (start, len <= 128), halves split at a multiple of 8;
//   * a leaf of len >= 8 is 8 accumulator chains r[j] = x[s+j] + x[s+8+j] + ... over the
//     len/8 full groups, combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the
//     len%8 tail elements added one by one; a leaf of len < 8 is a plain sequential sum;
//   * a postfix program over the leaves ((start, len) = push the leaf's sum, (-1, 0) =
//     pop two and push their sum); windows longer than numpy's 8192-element reduction
//     buffer are that recursion per 8192-element chunk, the chunks added in sequence.
// The kernel gives each chain (leaf, j) to one lane: 8 adjacent lanes (an "octet") run
// the 8 chains of a leaf side by side and combine them with three xor-butterfly
// exchanges (lane j adds lane j^1, then j^2, then j^4).  IEEE addition is commutative,
// so every lane of the octet ends with exactly ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)):
// the additions of the plan, in the plan's order, and nothing else.  plan_eval() below
// is the host evaluator of the same plan, lane for lane (rs_sad_plan_sum).
// rs_sad_scores, the score matrix of host arrays, is such a library for one call: every
// float score of the package is this plan's.
#include <climits>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "rs_common.h"

namespace {

// ---------------------------------------------------------------------------
// The plan
// ---------------------------------------------------------------------------
struct SadPlan {
    std::vector<int2> prog;   // postfix: (start, len) push leaf sum; (-1, 0) add
    int depth = 0;            // deepest stack the program needs
};

static void plan_rec(int64_t start, int64_t n, SadPlan& p, int sp, int& top) {
    if (n <= 128) {
        p.prog.push_back(make_int2((int)start, (int)n));
        if (sp + 1 > top) top = sp + 1;
        return;
    }
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    plan_rec(start, n2, p, sp, top);
    plan_rec(start + n2, n - n2, p, sp + 1, top);
    p.prog.push_back(make_int2(-1, 0));
}

// np.sum hands its inner loop at most NPY_CHUNK elements at a time (numpy's default
// reduction buffer, np.getbufsize() == 8192) and accumulates the chunks' pairwise sums
// one after the other: ((p0 + p1) + p2) + ...  Windows of up to 8192 elements are one chunk.
constexpr int64_t NPY_CHUNK = 8192;

static SadPlan make_plan(int64_t n) {
    SadPlan p;
    int top = 0;
    for (int64_t s = 0; s < n; s += NPY_CHUNK) {
        plan_rec(s, n - s < NPY_CHUNK ? n - s : NPY_CHUNK, p, s > 0 ? 1 : 0, top);
        if (s > 0) p.prog.push_back(make_int2(-1, 0));
    }
    p.depth = top;
    return p;
}

// Host evaluator: the plan executed as the kernel's lanes execute it.  x(i) is the
// i-th summand (|T - Q| of the flattened window, or a plain array element).
template <typename T, typename F>
static T plan_eval(const SadPlan& p, F x) {
    std::vector<T> st((size_t)p.depth + 1);
    int sp = 0;
    for (const int2& op : p.prog) {
        if (op.x < 0) {
            const T rhs = st[--sp];
            st[sp - 1] = st[sp - 1] + rhs;
            continue;
        }
        const int64_t s = op.x;
        const int len = op.y;
        T res;
        if (len < 8) {
            res = T(0);
            for (int k = 0; k < len; ++k) res += x(s + k);
        } else {
            const int nfull = len / 8;
            T lane[8];            // one chain per lane
            for (int j = 0; j < 8; ++j) {
                T r = x(s + j);
                for (int k = 1; k < nfull; ++k) r += x(s + 8 * k + j);
                lane[j] = r;
            }
            for (int m = 1; m < 8; m <<= 1) {   // the xor butterfly: lane j adds lane j^m
                T nxt[8];
                for (int j = 0; j < 8; ++j) nxt[j] = lane[j] + lane[j ^ m];
                for (int j = 0; j < 8; ++j) lane[j] = nxt[j];
            }
            res = lane[0];
            for (int k = 8 * nfull; k < len; ++k) res += x(s + k);
        }
        st[sp++] = res;
    }
    return st[0];
}

// ---------------------------------------------------------------------------
// Kernels
// ---------------------------------------------------------------------------
template <typename T>
__device__ inline T absdiff(T a, T b) {
    if constexpr (sizeof(T) == 4) return fabsf(a - b);   // numpy's absolute is fabs
    else return fabs(a - b);
}

template <typename T>
__device__ inline T xor_add(T v, int m) { return v + __shfl_xor(v, m, 64); }

// LDS address of template element e (flat index in the H x W template).  The octets of
// a wave read the same window one row (W elements) apart; with W * sizeof(T) a multiple
// of the 256-byte bank cycle they would all hit the same banks, so every 256 bytes of
// the tile are followed by 8 elements of padding: a row offset then also moves the
// bank.  Shifts only, for any W.  Global memory (PAD = false) is read in place.
template <typename T, bool PAD>
__device__ inline int tile_at(int e) {
    constexpr int LOG = sizeof(T) == 4 ? 6 : 5;
    return PAD ? e + ((e >> LOG) << 3) : e;
}

// K consecutive links of one chain: the K loads of either array are issued together,
// the additions then run in the chain's order.
template <typename T, bool PAD, int K>
__device__ inline T chain_links(T acc, const T* a, const T* b, int e, int i) {
    T x[K], y[K];
#pragma unroll
    for (int u = 0; u < K; ++u) {
        x[u] = a[tile_at<T, PAD>(e + 8 * u)];
        y[u] = b[i + 8 * u];
    }
#pragma unroll
    for (int u = 0; u < K; ++u) acc += absdiff(x[u], y[u]);
    return acc;
}

// One block scores template blockIdx.x against the queries of chunk blockIdx.y, `qt`
// queries per pass.  STAGED: the template (padded, tile_at) and the pass's query
// windows are copied to LDS with coalesced loads; the template tile stays for every
// query of the chunk and the 2M-1 offsets all read it.  !STAGED reads global memory
// in place (shapes whose tiles do not fit the LDS budget).
// Work item = (query of the pass, offset), one per octet; lane j of the octet owns the
// chains (leaf, j) of the plan, leaf after leaf; leaf sums go through a per-octet stack
// in LDS as the postfix program says.  A row offset o is a shift of o * W in the flat
// template, so element i of the window is template element (M + o) * W + i.
// out[q * ldo + t]; lower != 0 (in-batch matrix: the templates are the staged queries
// themselves) computes only t < q.
template <typename T, bool STAGED>
__global__ __launch_bounds__(256) void vtf_score_kernel(
    const T* __restrict__ lib, int64_t nt, const T* __restrict__ qry, int nq, int qchunk, int H,
    int W, int M, int tsize, int qt, int depth, const int2* __restrict__ prog, int nprog, int lower,
    int64_t ldo, T* __restrict__ out) {
    extern __shared__ double vtf_smem[];
    const int n = (H - 2 * M) * W, NO = 2 * M - 1;
    const int noct = blockDim.x >> 3, octet = threadIdx.x >> 3, j = threadIdx.x & 7;
    T* s_stack = reinterpret_cast<T*>(vtf_smem);            // [depth][noct]
    T* s_d = s_stack + (size_t)depth * noct;                // [qt][NO]
    T* s_t = s_d + (size_t)qt * NO;                         // [tsize]     (STAGED)
    T* s_q = s_t + (STAGED ? (size_t)tsize : 0);            // [qt][n]     (STAGED)
    const int64_t t = blockIdx.x;
    if (t >= nt) return;
    const int q0 = blockIdx.y * qchunk;
    const int q1 = min(nq, q0 + qchunk);
    if (lower && q1 - 1 <= t) {                             // nothing below the diagonal here
        for (int qi = q0 + (int)threadIdx.x; qi < q1; qi += blockDim.x)
            out[(size_t)qi * ldo + t] = T(INFINITY);
        return;
    }
    const T* gt = lib + (size_t)t * H * W;
    if (STAGED) {
#pragma unroll 4
        for (int e = threadIdx.x; e < H * W; e += blockDim.x) s_t[tile_at<T, true>(e)] = gt[e];
    }
    for (int qb = q0; qb < q1; qb += qt) {
        const int nqp = min(qt, q1 - qb);
        if (STAGED) {
            for (int k = 0; k < nqp; ++k) {
                const T* gq = qry + (size_t)(qb + k) * H * W + (size_t)M * W;
#pragma unroll 4
                for (int i = threadIdx.x; i < n; i += blockDim.x) s_q[k * n + i] = gq[i];
            }
        }
        __syncthreads();
        for (int w = octet; w < nqp * NO; w += noct) {
            const int k = w / NO, oi = w - k * NO, qi = qb + k;
            T d = T(INFINITY);
            if (!(lower && qi <= t)) {
                const T* a = STAGED ? s_t : gt;                       // template (tile_at)
                const T* b = STAGED ? s_q + (size_t)k * n             // query window, flat
                                    : qry + (size_t)qi * H * W + (size_t)M * W;
                const int e0 = (oi + 1) * W;                          // (M + o) * W, o = oi - (M-1)
                int sp = 0;
                int2 nxt = prog[0];
                for (int p = 0; p < nprog; ++p) {
                    const int2 op = nxt;
                    if (p + 1 < nprog) nxt = prog[p + 1];
                    if (op.x < 0) {
                        --sp;
                        const T rhs = s_stack[sp * noct + octet];
                        s_stack[(sp - 1) * noct + octet] = s_stack[(sp - 1) * noct + octet] + rhs;
                        continue;
                    }
                    const int s = op.x, len = op.y;
                    T res;
                    if (len < 8) {
                        res = T(0);
                        for (int u = 0; u < len; ++u)
                            res += absdiff(a[tile_at<T, STAGED>(e0 + s + u)], b[s + u]);
                    } else {
                        const int nfull = len >> 3;
                        int i = s + j, e = e0 + i;
                        T acc = absdiff(a[tile_at<T, STAGED>(e)], b[i]);
                        int g = 1;
                        for (; g + 8 <= nfull; g += 8)
                            acc = chain_links<T, STAGED, 8>(acc, a, b, e + 8 * g, i + 8 * g);
                        if (g + 4 <= nfull) {
                            acc = chain_links<T, STAGED, 4>(acc, a, b, e + 8 * g, i + 8 * g);
                            g += 4;
                        }
                        if (g + 2 <= nfull) {
                            acc = chain_links<T, STAGED, 2>(acc, a, b, e + 8 * g, i + 8 * g);
                            g += 2;
                        }
                        if (g < nfull) acc = chain_links<T, STAGED, 1>(acc, a, b, e + 8 * g, i + 8 * g);
                        acc = xor_add(acc, 1);
                        acc = xor_add(acc, 2);
                        acc = xor_add(acc, 4);
                        res = acc;
                        for (int u = nfull * 8; u < len; ++u)
                            res += absdiff(a[tile_at<T, STAGED>(e0 + s + u)], b[s + u]);
                    }
                    s_stack[sp * noct + octet] = res;
                    ++sp;
                }
                d = s_stack[octet];
            }
            if (j == 0) s_d[k * NO + oi] = d;
        }
        __syncthreads();
        if ((int)threadIdx.x < nqp) {
            // `if diff < mindiff` from +inf over the offsets in order: a NaN is never taken
            T best = T(INFINITY);
            for (int oi = 0; oi < NO; ++oi) {
                const T v = s_d[threadIdx.x * NO + oi];
                if (v < best) best = v;
            }
            out[(size_t)(qb + threadIdx.x) * ldo + t] = best;
        }
        // the next pass stages s_q (not read by the min threads) and writes s_d only
        // after its own barrier
    }
}

// (min score, first argmin) of one query's row of scores.  Scores are >= +0 or +inf,
// so their bit patterns order as unsigned integers; the (bits, index) key is compared
// lexicographically, which is np.argmin's first minimum, ties and all-inf rows included.
template <typename T>
__global__ __launch_bounds__(256) void vtf_argmin_kernel(const T* __restrict__ scores, int64_t nt,
                                                         T* __restrict__ best,
                                                         int64_t* __restrict__ bidx) {
    __shared__ unsigned long long s_b[256];
    __shared__ long long s_i[256];
    const T* row = scores + (size_t)blockIdx.x * nt;
    unsigned long long kb = ~0ull;
    long long ki = 0x7fffffffffffffffll;
    for (int64_t t = threadIdx.x; t < nt; t += 256) {
        unsigned long long b;
        if constexpr (sizeof(T) == 4) b = __float_as_uint(row[t]);
        else b = (unsigned long long)__double_as_longlong(row[t]);
        if (b < kb) { kb = b; ki = t; }   // t ascends per thread: the first of equal bits stays
    }
    s_b[threadIdx.x] = kb;
    s_i[threadIdx.x] = ki;
    __syncthreads();
    for (int m = 128; m > 0; m >>= 1) {
        if ((int)threadIdx.x < m) {
            const unsigned long long ob = s_b[threadIdx.x + m];
            const long long oi = s_i[threadIdx.x + m];
            if (ob < s_b[threadIdx.x] || (ob == s_b[threadIdx.x] && oi < s_i[threadIdx.x])) {
                s_b[threadIdx.x] = ob;
                s_i[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if constexpr (sizeof(T) == 4) best[blockIdx.x] = __uint_as_float((unsigned)s_b[0]);
        else best[blockIdx.x] = __longlong_as_double((long long)s_b[0]);
        bidx[blockIdx.x] = s_i[0];
    }
}

constexpr size_t LDS_BUDGET = 64 * 1024;

}  // namespace

// ===========================================================================
// Host side
// ===========================================================================
// The buffers are rs::DevBuf members (rs_common.h; untyped ones count bytes, the element
// being es wide).  Group capacities: qCap (dQ), scanCap (dIn, dBest, dBidx).  The stream
// and the events are rs::Stream / rs::Event owners.
struct rs_vtf {
    int H = 0, W = 0, M = 0, dtype = 0, device = 0;
    size_t es = 0;            // element size
    int64_t count = 0, cap = 0;   // templates stored, and templates dLib holds
    rs::DevBuf<void> dLib;
    SadPlan plan;
    rs::DevBuf<int2> dProg;
    // launch shape of the score kernel
    bool staged = false;      // template and query tiles fit the LDS budget
    int tsize = 0;            // elements of the padded template tile (tile_at)
    // staged queries and results
    int qCap = 0, nqStaged = 0, scanCap = 0;
    rs::DevBuf<void> dQ;
    rs::DevBuf<void> dIn;        // [scanCap][scanCap] in-batch scores
    rs::DevBuf<void> dBest;      // [scanCap]
    rs::DevBuf<int64_t> dBidx;   // [scanCap]
    rs::DevBuf<void> dScores;    // (its capacity in bytes)
    bool timing = false;
    double lastMs = -1.0;
    // the owners come after the buffers: members go in reverse order, streams and events first
    rs::Stream stream;
    rs::Event ev0, ev1;
};

namespace {

size_t lds_bytes(const rs_vtf* h, int threads, int qt, bool staged) {
    const size_t n = (size_t)(h->H - 2 * h->M) * h->W;
    size_t el = (size_t)h->plan.depth * (threads / 8) + (size_t)qt * (2 * h->M - 1);
    if (staged) el += (size_t)h->tsize + (size_t)qt * n;
    return el * h->es;
}

int ensure_lib(rs_vtf* h, int64_t want) {
    if (want <= h->cap) return RS_OK;
    const int64_t cap = rs::grown<int64_t>(h->cap, want, 1);
    const size_t tb = (size_t)h->H * h->W * h->es;
    rs::DevBuf<void> nl;   // the library is copied: the new block before the old one goes
    RS_TRY(nl.reserve((size_t)cap * tb, "float template library"));
    if (h->count > 0) {
        RS_HIP(hipMemcpyAsync(nl.get(), h->dLib.get(), (size_t)h->count * tb, hipMemcpyDeviceToDevice, h->stream.get()));
        RS_HIP(hipStreamSynchronize(h->stream.get()));
    }
    h->dLib = std::move(nl);
    h->cap = cap;
    return RS_OK;
}

int ensure_queries(rs_vtf* h, int nq) {
    if (nq <= h->qCap) return RS_OK;
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    const int cap = rs::grown(h->qCap, nq, 1);
    h->qCap = 0;
    h->nqStaged = 0;
    RS_TRY(h->dQ.reserve((size_t)cap * h->H * h->W * h->es));
    h->qCap = cap;
    return RS_OK;
}

// what rs_vtf_scan alone writes: a handle that only scores (rs_sad_scores' is one) never
// allocates them
int ensure_scan_results(rs_vtf* h, int nq) {
    if (nq <= h->scanCap) return RS_OK;
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    const int cap = rs::grown(h->scanCap, nq, 1);
    h->scanCap = 0;
    RS_TRY(h->dIn.reserve((size_t)cap * cap * h->es));
    RS_TRY(h->dBest.reserve((size_t)cap * h->es));
    RS_TRY(h->dBidx.reserve((size_t)cap));
    h->scanCap = cap;
    return RS_OK;
}

int ensure_scores(rs_vtf* h, size_t elems) {
    if (elems * h->es <= h->dScores.capacity()) return RS_OK;
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    return h->dScores.reserve(elems * h->es);
}

int stage_queries(rs_vtf* h, int nq, const void* queries) {
    RS_TRY(ensure_queries(h, nq));
    RS_HIP(hipMemcpyAsync(h->dQ.get(), queries, (size_t)nq * h->H * h->W * h->es, hipMemcpyHostToDevice,
                          h->stream.get()));
    h->nqStaged = nq;
    return RS_OK;
}

// scores of the staged queries [0, nq) against nt templates at `lib` -> out[q * nt + t]
template <typename T>
int launch_scores(rs_vtf* h, const void* lib, int64_t nt, int nq, int lower, void* out) {
    const int NO = 2 * h->M - 1;
    const int qt = nq >= 2 ? 2 : 1;
    const int threads = qt * NO <= 16 ? 128 : 256;
    // enough blocks to fill the device when the library is small; otherwise one chunk,
    // so that a template tile is staged once for the whole batch
    int64_t chunks = (1024 + nt - 1) / nt;
    const int64_t maxChunks = (nq + qt - 1) / qt;
    if (chunks > maxChunks) chunks = maxChunks;
    if (chunks < 1) chunks = 1;
    int qchunk = (int)((nq + chunks - 1) / chunks);
    qchunk = (qchunk + qt - 1) / qt * qt;
    chunks = (nq + qchunk - 1) / qchunk;
    RS_CHECK(nt < (1ll << 31) && chunks <= 65535, RS_ERR_ARG, "too many templates or queries");
    const size_t lds = lds_bytes(h, threads, qt, h->staged);
    RS_CHECK(lds <= LDS_BUDGET, RS_ERR_ARG, "window too deep for the scan's LDS stack");
    const dim3 grid((unsigned)nt, (unsigned)chunks);
    const int n_prog = (int)h->plan.prog.size();
    if (h->staged)
        hipLaunchKernelGGL((vtf_score_kernel<T, true>), grid, dim3(threads), lds, h->stream.get(),
                           static_cast<const T*>(lib), nt, static_cast<const T*>(h->dQ.get()), nq, qchunk,
                           h->H, h->W, h->M, h->tsize, qt, h->plan.depth, h->dProg.get(), n_prog, lower, nt,
                           static_cast<T*>(out));
    else
        hipLaunchKernelGGL((vtf_score_kernel<T, false>), grid, dim3(threads), lds, h->stream.get(),
                           static_cast<const T*>(lib), nt, static_cast<const T*>(h->dQ.get()), nq, qchunk,
                           h->H, h->W, h->M, 0, qt, h->plan.depth, h->dProg.get(), n_prog, lower, nt,
                           static_cast<T*>(out));
    RS_HIP(hipGetLastError());
    return RS_OK;
}

int launch_scores(rs_vtf* h, const void* lib, int64_t nt, int nq, int lower, void* out) {
    return h->dtype == RS_DT_F32 ? launch_scores<float>(h, lib, nt, nq, lower, out)
                                 : launch_scores<double>(h, lib, nt, nq, lower, out);
}

int launch_argmin(rs_vtf* h, int nq, int64_t nt) {
    if (h->dtype == RS_DT_F32)
        hipLaunchKernelGGL(vtf_argmin_kernel<float>, dim3(nq), dim3(256), 0, h->stream.get(),
                           static_cast<const float*>(h->dScores.get()), nt, static_cast<float*>(h->dBest.get()),
                           h->dBidx.get());
    else
        hipLaunchKernelGGL(vtf_argmin_kernel<double>, dim3(nq), dim3(256), 0, h->stream.get(),
                           static_cast<const double*>(h->dScores.get()), nt,
                           static_cast<double*>(h->dBest.get()), h->dBidx.get());
    RS_HIP(hipGetLastError());
    return RS_OK;
}

// what a library (rs_vtf_create) and a one-off score matrix (rs_sad_scores) accept
int check_geometry(int dtype, int H, int W, int max_offset) {
    RS_CHECK(dtype == RS_DT_F32 || dtype == RS_DT_F64, RS_ERR_TYPE, "dtype %d is not F32/F64", dtype);
    RS_CHECK(H > 0 && W > 0 && max_offset >= 1 && max_offset <= 16 && H > 2 * max_offset,
             RS_ERR_ARG, "bad shape (%d, %d) for max_offset %d", H, W, max_offset);
    RS_CHECK((int64_t)H * W <= (1ll << 30), RS_ERR_ARG, "template too large");
    return RS_OK;
}

void fill_inf(int dtype, void* p, size_t n) {
    if (dtype == RS_DT_F32)
        for (size_t i = 0; i < n; ++i) static_cast<float*>(p)[i] = std::numeric_limits<float>::infinity();
    else
        for (size_t i = 0; i < n; ++i) static_cast<double*>(p)[i] = std::numeric_limits<double>::infinity();
}

}  // namespace

extern "C" {

int rs_vtf_create(int H, int W, int max_offset, int dtype, int64_t capacity, int device,
                  rs_vtf** out) {
    rs::clear_error();
    RS_CHECK(out != nullptr, RS_ERR_ARG, "null output handle");
    *out = nullptr;
    RS_TRY(check_geometry(dtype, H, W, max_offset));
    RS_CHECK(capacity >= 0, RS_ERR_ARG, "negative capacity");
    RS_TRY(rs::use_device(device));
    // one failure exit: rs_vtf_destroy takes a handle at any stage
    std::unique_ptr<rs_vtf, int (*)(rs_vtf*)> owner(new rs_vtf(), rs_vtf_destroy);
    rs_vtf* const h = owner.get();
    h->H = H; h->W = W; h->M = max_offset; h->dtype = dtype; h->device = device;
    h->es = dtype == RS_DT_F32 ? 4 : 8;
    h->plan = make_plan((int64_t)(H - 2 * max_offset) * W);
    // the padded template tile (tile_at): 8 elements after every 256 bytes
    const int64_t hw = (int64_t)H * W;
    const int64_t tsize = hw + ((hw >> (dtype == RS_DT_F32 ? 6 : 5)) << 3) + 8;
    h->tsize = (int)(tsize < (1 << 24) ? tsize : (1 << 24));
    h->staged = tsize < (1 << 24) && lds_bytes(h, 256, 2, true) <= LDS_BUDGET;
    RS_CHECK(lds_bytes(h, 256, 2, false) <= LDS_BUDGET, RS_ERR_ARG, "window too deep for the scan's LDS stack");
    RS_TRY(h->stream.create());
    RS_TRY(h->dProg.reserve(h->plan.prog.size()));
    RS_HIP(hipMemcpyAsync(h->dProg.get(), h->plan.prog.data(), sizeof(int2) * h->plan.prog.size(),
                          hipMemcpyHostToDevice, h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    RS_TRY(h->ev0.create());
    RS_TRY(h->ev1.create());
    RS_TRY(ensure_lib(h, capacity > 0 ? capacity : 1));
    *out = owner.release();
    return RS_OK;
}

int rs_vtf_destroy(rs_vtf* h) {
    if (!h) return RS_OK;
    (void)hipSetDevice(h->device);
    // queued work that failed after a call returned is reported here, not dropped
    const hipError_t se = rs::sync_streams({h->stream.get()});
    delete h;  // (the streams and events, then the buffers, go with their members)
    RS_CHECK(se == hipSuccess, RS_ERR_HIP, "work queued before rs_vtf_destroy failed: %s", hipGetErrorString(se));
    return RS_OK;
}

int rs_vtf_count(const rs_vtf* h, int64_t* count) {
    rs::clear_error();
    RS_CHECK(h && count, RS_ERR_ARG, "null argument");
    *count = h->count;
    return RS_OK;
}

int rs_vtf_add(rs_vtf* h, int n, const void* templates, int64_t* first_index) {
    rs::clear_error();
    RS_CHECK(h != nullptr, RS_ERR_ARG, "null handle");
    RS_CHECK(n >= 0, RS_ERR_ARG, "negative count");
    if (first_index) *first_index = h->count;
    if (n == 0) return RS_OK;
    RS_CHECK(templates != nullptr, RS_ERR_ARG, "null templates");
    RS_HIP(hipSetDevice(h->device));
    RS_TRY(ensure_lib(h, h->count + n));
    const size_t tb = (size_t)h->H * h->W * h->es;
    RS_HIP(hipMemcpyAsync(static_cast<char*>(h->dLib.get()) + (size_t)h->count * tb, templates,
                          (size_t)n * tb, hipMemcpyHostToDevice, h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    h->count += n;
    return RS_OK;
}

int rs_vtf_read(rs_vtf* h, int64_t index, void* out) {
    rs::clear_error();
    RS_CHECK(h && out, RS_ERR_ARG, "null argument");
    RS_CHECK(index >= 0 && index < h->count, RS_ERR_ARG, "template %lld not in [0, %lld)",
             (long long)index, (long long)h->count);
    RS_HIP(hipSetDevice(h->device));
    const size_t tb = (size_t)h->H * h->W * h->es;
    RS_HIP(hipMemcpyAsync(out, static_cast<char*>(h->dLib.get()) + (size_t)index * tb, tb,
                          hipMemcpyDeviceToHost, h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    return RS_OK;
}

int rs_vtf_scores(rs_vtf* h, int nq, const void* queries, int64_t t0, int64_t nt, void* scores) {
    rs::clear_error();
    RS_CHECK(h != nullptr, RS_ERR_ARG, "null handle");
    RS_CHECK(nq >= 0 && t0 >= 0 && nt >= 0 && t0 + nt <= h->count, RS_ERR_ARG,
             "templates [%lld, %lld) not in [0, %lld)", (long long)t0, (long long)(t0 + nt),
             (long long)h->count);
    if (nq == 0 || nt == 0) return RS_OK;
    RS_CHECK(queries && scores, RS_ERR_ARG, "null argument");
    RS_HIP(hipSetDevice(h->device));
    RS_TRY(stage_queries(h, nq, queries));
    RS_TRY(ensure_scores(h, (size_t)nq * nt));
    const size_t tb = (size_t)h->H * h->W * h->es;
    RS_TRY(launch_scores(h, static_cast<char*>(h->dLib.get()) + (size_t)t0 * tb, nt, nq, 0, h->dScores.get()));
    RS_HIP(hipMemcpyAsync(scores, h->dScores.get(), (size_t)nq * nt * h->es, hipMemcpyDeviceToHost,
                          h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    return RS_OK;
}

int rs_vtf_scan(rs_vtf* h, int nq, const void* queries, int want_inbatch, void* best_score,
                int64_t* best_index, void* inbatch) {
    rs::clear_error();
    RS_CHECK(h != nullptr, RS_ERR_ARG, "null handle");
    RS_CHECK(nq >= 0, RS_ERR_ARG, "negative count");
    h->lastMs = -1.0;
    if (nq == 0) return RS_OK;
    RS_CHECK(queries && best_score && best_index, RS_ERR_ARG, "null argument");
    RS_CHECK(!want_inbatch || inbatch, RS_ERR_ARG, "null in-batch matrix");
    RS_HIP(hipSetDevice(h->device));
    RS_TRY(stage_queries(h, nq, queries));
    RS_TRY(ensure_scan_results(h, nq));
    const int64_t nt = h->count;
    if (nt > 0) {
        RS_TRY(ensure_scores(h, (size_t)nq * nt));
        if (h->timing) RS_HIP(hipEventRecord(h->ev0.get(), h->stream.get()));
        RS_TRY(launch_scores(h, h->dLib.get(), nt, nq, 0, h->dScores.get()));
        RS_TRY(launch_argmin(h, nq, nt));
        if (h->timing) RS_HIP(hipEventRecord(h->ev1.get(), h->stream.get()));
        RS_HIP(hipMemcpyAsync(best_score, h->dBest.get(), (size_t)nq * h->es, hipMemcpyDeviceToHost,
                              h->stream.get()));
        RS_HIP(hipMemcpyAsync(best_index, h->dBidx.get(), (size_t)nq * sizeof(int64_t),
                              hipMemcpyDeviceToHost, h->stream.get()));
    }
    if (want_inbatch) {
        RS_TRY(launch_scores(h, h->dQ.get(), nq, nq, 1, h->dIn.get()));
        RS_HIP(hipMemcpyAsync(inbatch, h->dIn.get(), (size_t)nq * nq * h->es, hipMemcpyDeviceToHost,
                              h->stream.get()));
    }
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    if (nt == 0) {
        fill_inf(h->dtype, best_score, (size_t)nq);
        for (int i = 0; i < nq; ++i) best_index[i] = -1;
    } else if (h->timing) {
        float ms = 0.f;
        RS_HIP(hipEventElapsedTime(&ms, h->ev0.get(), h->ev1.get()));
        h->lastMs = ms;
    }
    return RS_OK;
}

int rs_vtf_append_staged(rs_vtf* h, int n, const int32_t* which, int64_t* first_index) {
    rs::clear_error();
    RS_CHECK(h != nullptr, RS_ERR_ARG, "null handle");
    RS_CHECK(n >= 0, RS_ERR_ARG, "negative count");
    if (first_index) *first_index = h->count;
    if (n == 0) return RS_OK;
    RS_CHECK(which != nullptr, RS_ERR_ARG, "null index list");
    for (int i = 0; i < n; ++i)
        RS_CHECK(which[i] >= 0 && which[i] < h->nqStaged, RS_ERR_ARG,
                 "staged query %d not in [0, %d)", which[i], h->nqStaged);
    RS_HIP(hipSetDevice(h->device));
    RS_TRY(ensure_lib(h, h->count + n));
    const size_t tb = (size_t)h->H * h->W * h->es;
    for (int i = 0; i < n;) {
        int run = 1;   // consecutive staged queries go as one copy
        while (i + run < n && which[i + run] == which[i] + run) ++run;
        RS_HIP(hipMemcpyAsync(static_cast<char*>(h->dLib.get()) + (size_t)(h->count + i) * tb,
                              static_cast<char*>(h->dQ.get()) + (size_t)which[i] * tb, (size_t)run * tb,
                              hipMemcpyDeviceToDevice, h->stream.get()));
        i += run;
    }
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    h->count += n;
    return RS_OK;
}

int rs_vtf_set_timing(rs_vtf* h, int enable) {
    rs::clear_error();
    RS_CHECK(h != nullptr, RS_ERR_ARG, "null handle");
    h->timing = enable != 0;
    h->lastMs = -1.0;
    return RS_OK;
}

int rs_vtf_last_ms(rs_vtf* h, double* ms) {
    rs::clear_error();
    RS_CHECK(h && ms, RS_ERR_ARG, "null argument");
    *ms = h->lastMs;
    return RS_OK;
}

// The score matrix of host arrays: a library for the duration of the call, so the one plan
// and the one kernel of the resident path (out[q * nt + t], as rs_vtf_scores lays it out).
int rs_sad_scores(int device, int dtype, int H, int W, int max_offset, int64_t nt,
                  const void* templates, int nq, const void* queries, void* scores) {
    rs::clear_error();
    RS_TRY(check_geometry(dtype, H, W, max_offset));
    RS_CHECK(nt >= 0 && nq >= 0, RS_ERR_ARG, "negative count");
    if (nt == 0 || nq == 0) return RS_OK;
    RS_CHECK(templates && queries && scores, RS_ERR_ARG, "null argument");
    RS_CHECK(nt <= INT_MAX, RS_ERR_ARG, "too many templates");
    rs_vtf* h = nullptr;
    RS_TRY(rs_vtf_create(H, W, max_offset, dtype, nt, device, &h));
    int rc = rs_vtf_add(h, (int)nt, templates, nullptr);
    if (rc == RS_OK) rc = rs_vtf_scores(h, nq, queries, 0, nt, scores);
    const int freed = rs_vtf_destroy(h);   // (a failure's message stays: destroy does not clear it)
    return rc != RS_OK ? rc : freed;
}

int rs_sad_plan_sum(int dtype, int64_t n, const void* values, void* out) {
    rs::clear_error();
    RS_CHECK(dtype == RS_DT_F32 || dtype == RS_DT_F64, RS_ERR_TYPE, "dtype %d is not F32/F64", dtype);
    RS_CHECK(n >= 1 && n <= (1ll << 30), RS_ERR_ARG, "n = %lld not in [1, 2^30]", (long long)n);
    RS_CHECK(values && out, RS_ERR_ARG, "null argument");
    const SadPlan plan = make_plan(n);
    if (dtype == RS_DT_F32) {
        const float* x = static_cast<const float*>(values);
        *static_cast<float*>(out) = plan_eval<float>(plan, [x](int64_t i) { return x[i]; });
    } else {
        const double* x = static_cast<const double*>(values);
        *static_cast<double*>(out) = plan_eval<double>(plan, [x](int64_t i) { return x[i]; });
    }
    return RS_OK;
}

}  // extern "C"
