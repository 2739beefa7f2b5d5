// Generic per-node path: graphs the recognisers (pyvb_amd/_recognise.py) have no fused plan for run node by node.
// Every quantity of such a graph -- posterior parameters, constants, messages, temporaries -- lives in one device
// arena of doubles; what a node's update(), pass_up_m1_m2(), pass_down_*() or log_lower_bound() computes in the reference
// (gaussian.py:102-183, node.py:95-129,182-276, nodes_todo.py:33-62,125-157,183-204,224-234) is emitted by the host
// (pyvb_amd/generic.py) as a TAPE of small dense operations on arena offsets, and one workgroup interprets the tape:
// one launch per node update, or per whole Network.learn iteration, instead of one launch per numpy call.
// The matrices of this path are tiny (dimensions of single nodes); the interpreter favours generality over speed.
#include "common.h"
#include "digamma.h"         // digamma_pos: U_DIGAMMA
#include "tape_plan.h"          // tape.h: opcodes, record layout, the window form

#define TAPE_CTHREADS (64 * TAPE_BUNDLE)

struct TapeArgs { double* arena; size_t arena_n; const int* ops; int nops; int* status; };

#define TAPE_THREADS 256    // (one wavefront, 64, measured the same on the node-sized matrices of this path: the barrier per record is not what a record costs)

// `count` records starting at `recs` (global memory, or a chunk staged in LDS), interpreted by the calling workgroup.
// WIN: every operand of every record lies in the workgroup's LDS window `win` (the offsets are window positions, tagged
// T_LDS); the pointers are then LDS pointers and the accesses ds_read / ds_write (a few dozen cycles) instead of flat ones.
typedef __attribute__((address_space(3))) double lds_double;
template <bool WIN> struct TapePtr { typedef double* type; };
template <> struct TapePtr<true> { typedef lds_double* type; };

// NT: threads of the workgroup.  NT == 64 (one wavefront; the host picks it for launches whose records all have at most 64
// elements, WIN only) needs no s_barrier between records: the LDS operations of a wavefront execute in order, a fence keeps the
// compiler from moving them.  What a record of a node-sized graph costs is its chain of dependent steps -- fetch the record,
// form the addresses, fetch the operands, store -- so: the record is fetched as two 16-byte words one record ahead, and the
// row / column of an element comes from a float reciprocal with a fix-up instead of two integer divisions (about 80 instructions).
typedef int __attribute__((ext_vector_type(4))) tape_i4;
// exact for idx < TAPE_MAX_ELEMS (the derivation is in tape.h; tape_describe admits no larger record of the opcodes that call it)
__device__ __forceinline__ void tape_divmod(int idx, int n, float rn, int& i, int& j) {
    i = (int)(((float)idx + 0.5f) * rn);
    j = idx - i * n;
    if (j < 0) { --i; j += n; } else if (j >= n) { ++i; j -= n; }
}

template <bool WIN, int NT>
__device__ static void tape_exec(const TapeArgs& t, const int* recs, int count, double* red, typename TapePtr<WIN>::type win, const int tid) {
    typedef typename TapePtr<WIN>::type P;
    double* A = t.arena;
    auto at = [&](int off) -> P { if constexpr (WIN) return win + (off & ~T_LDS); else return A + off; };
    auto sync = [&]() {
        if constexpr (NT == 64 && WIN) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        } else __syncthreads();
    };
    const tape_i4* r4 = reinterpret_cast<const tape_i4*>(recs);
    tape_i4 nlo = r4[0], nhi = r4[1];
    for (int pc = 0; pc < count; ++pc) {
        const tape_i4 lo = nlo, hi = nhi;
        if (pc + 1 < count) { nlo = r4[2 * pc + 2]; nhi = r4[2 * pc + 3]; }
        const int o[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        const int op = o[0], m = o[4], n = o[5], flags = o[7];
        const float rn = __builtin_amdgcn_rcpf((float)(n > 0 ? n : 1));
        P dst = at(o[1]);
        const P a = at(o[2]);
        const P b = o[3] < 0 ? at(0) : at(o[3]);
        switch (op) {
        case T_COPY2D:
            for (int idx = tid; idx < m * n; idx += NT) { int i, j; tape_divmod(idx, n, rn, i, j); dst[i * o[3] + j] = a[i * o[6] + j]; }
            break;
        case T_FILL:
            for (int idx = tid; idx < m * n; idx += NT) { int i, j; tape_divmod(idx, n, rn, i, j); dst[i * o[3] + j] = ((flags & 1) && i == j) ? 1.0 : 0.0; }
            break;
        case T_AXPBY: {
            const double al = *at(o[6]);
            if (o[3] < 0) { for (int idx = tid; idx < m * n; idx += NT) dst[idx] = al * a[idx]; }
            else { const double be = *at(flags); for (int idx = tid; idx < m * n; idx += NT) dst[idx] = al * a[idx] + be * b[idx]; }
            break; }
        case T_GEMM: {
            const int k = o[6];
            // strides instead of a choice per term, and eight terms fetched at a time: the sum over the children of a node
            // with thousands of them is one such product with a row of ones, a load latency per term otherwise
            const int as = (flags & 1) ? m : 1, bs = (flags & 2) ? 1 : n;
            auto part_sum = [&](int i, int j, int l0, int step) {      // terms l0, l0 + step, ... of element (i, j), in that order
                const P ap = a + ((flags & 1) ? i : i * k), bp = b + ((flags & 2) ? j * k : j);
                double s = 0.0;
                int l = l0;
                for (; l + 7 * step < k; l += 8 * step) {
                    double av[8], bv[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) { av[u] = ap[(l + u * step) * as]; bv[u] = bp[(l + u * step) * bs]; }
#pragma unroll
                    for (int u = 0; u < 8; ++u) s += av[u] * bv[u];
                }
                for (; l < k; l += step) s += ap[l * as] * bp[l * bs];
                return s;
            };
            if (k >= 64 && 2 * m * n <= NT) {
                // a long sum into few elements (the messages of thousands of children, the terms of a bound): every element's
                // terms are split over PL neighbouring lanes of a wavefront -- lane p takes terms p, p + PL, ... -- and the PL
                // partial sums are added in a fixed tree (shuffles): deterministic, but not the order of a chain of additions
                int PL = 64;
                while (PL * m * n > NT) PL >>= 1;
                {
                    const int e = tid / PL, p0 = tid % PL;
                    const bool live = e < m * n;
                    int i = 0, j = 0;
                    if (live) tape_divmod(e, n, rn, i, j);
                    double s = live ? part_sum(i, j, p0, PL) : 0.0;
                    for (int sh = PL >> 1; sh > 0; sh >>= 1) s += __shfl_xor(s, sh, 64);
                    if (live && p0 == 0) {
                        if (flags & 8) s = -s;
                        dst[e] = (flags & 4) ? dst[e] + s : s;
                    }
                }
                break;
            }
            for (int idx = tid; idx < m * n; idx += NT) {
                int i, j; tape_divmod(idx, n, rn, i, j);
                double s = part_sum(i, j, 0, 1);
                if (flags & 8) s = -s;
                dst[idx] = (flags & 4) ? dst[idx] + s : s;
            }
            break; }
        case T_SCALE: {
            const double s = *b;
            for (int idx = tid; idx < m * n; idx += NT) dst[idx] = (flags & 1) ? a[idx] / s : a[idx] * s;
            break; }
        case T_TRACE: case T_DOT: {
            double s = 0.0;
            if (op == T_TRACE) { for (int i = tid; i < m; i += NT) s += a[i * m + i]; }
            else { for (int idx = tid; idx < m * n; idx += NT) s += a[idx] * b[idx]; }
            // fixed tree: shuffles inside a wavefront, then the wavefronts in order (one thread adding up 256 values was
            // 7 us per record)
#pragma unroll
            for (int sh = 32; sh > 0; sh >>= 1) s += __shfl_xor(s, sh, 64);
            if constexpr (NT == 64) {
                if (tid == 0) dst[0] = (flags & 4) ? dst[0] + s : s;
            } else {
                if ((tid & 63) == 0) red[tid >> 6] = s;
                __syncthreads();
                if (tid == 0) {
                    double tot = 0.0;
#pragma unroll
                    for (int w = 0; w < NT / 64; ++w) tot += red[w];
                    dst[0] = (flags & 4) ? dst[0] + tot : tot;
                }
            }
            break; }
        case T_DIAG:
            if (flags & 1) { const float rm = __builtin_amdgcn_rcpf((float)(m > 0 ? m : 1)); for (int idx = tid; idx < m * m; idx += NT) { int i, j; tape_divmod(idx, m, rm, i, j); dst[idx] = (i == j) ? a[i] : 0.0; } }
            else { for (int i = tid; i < m; i += NT) dst[i] = a[i * m + i]; }
            break;
        case T_CHOLINV: {
            // L (lower, row major) in scratch, column by column; then X = L^{-1} by forward substitution, one thread per
            // column of the identity; then dst = X^T X.  (cho_factor / cho_solve of gaussian.py:118-119.)
            P L = at(o[6]);
            P X = L + m * m;
            P out2 = at(o[3]);
            for (int idx = tid; idx < m * m; idx += NT) L[idx] = a[idx];
            sync();
            for (int j = 0; j < m; ++j) {
                if (tid == 0) {
                    const double piv = L[j * m + j];
                    if (!(piv > 0.0)) { atomicOr(t.status, 1); L[j * m + j] = nan(""); }
                    else L[j * m + j] = sqrt(piv);
                }
                sync();
                const double d = L[j * m + j];
                for (int i = j + 1 + tid; i < m; i += NT) L[i * m + j] /= d;
                sync();
                const int rem = m - j - 1;                      // trailing update, lower triangle
                const float rr = __builtin_amdgcn_rcpf((float)(rem > 0 ? rem : 1));
                for (int idx = tid; idx < rem * rem; idx += NT) {
                    int i, c; tape_divmod(idx, rem, rr, i, c); i += j + 1; c += j + 1;
                    if (c <= i) L[i * m + c] -= L[i * m + j] * L[c * m + j];
                }
                sync();
            }
            if (tid == 0) {
                double s = 0.0;
                for (int j = 0; j < m; ++j) s += log(L[j * m + j]);
                out2[0] = 0.5 / s;          // gaussian.py:120: .5 / np.log(np.prod(np.diag(chol)))
                out2[1] = s;
            }
            for (int c = tid; c < m; c += NT) {       // X[:, c] = L^{-1} e_c
                for (int i = 0; i < m; ++i) {
                    double s = (i == c) ? 1.0 : 0.0;
                    for (int l = c; l < i; ++l) s -= L[i * m + l] * X[l * m + c];
                    X[i * m + c] = (i < c) ? 0.0 : s / L[i * m + i];
                }
            }
            sync();
            const float rm = __builtin_amdgcn_rcpf((float)(m > 0 ? m : 1));
            for (int idx = tid; idx < m * m; idx += NT) {
                int i, j; tape_divmod(idx, m, rm, i, j);
                double s = 0.0;
                for (int l = (i > j ? i : j); l < m; ++l) s += X[l * m + i] * X[l * m + j];
                dst[idx] = s;
            }
            break; }
        case T_UNARY:
            for (int idx = tid; idx < m * n; idx += NT) {
                const double x = a[idx];
                double y;
                switch (flags) {
                    case 0: y = log(x); break;
                    case 1: y = digamma_pos(x); break;
                    case 2: y = lgamma(x); break;
                    case 3: y = 1.0 / x; break;
                    case 4: y = -x; break;
                    default: y = exp(x); break;
                }
                dst[idx] = y;
            }
            break;
        case T_GATHER:          // the indices are data: checked here (status bit 1), everything else in pyvb_graph_tape_create
            for (int idx = tid; idx < m * n; idx += NT) {
                const long pos = (long)o[2] + (long)A[o[3] + idx / n] * o[6] + (long)A[flags + idx % n];
                if (pos < 0 || (size_t)pos >= t.arena_n) { atomicOr(t.status, 2); continue; }
                dst[idx] = A[pos];
            }
            break;
        case T_SCATTER:
            for (int idx = tid; idx < m * n; idx += NT) {
                const long pos = (long)o[1] + (long)A[o[3] + idx / n] * o[6] + (long)A[(flags & ~T_ACC) + idx % n];
                if (pos < 0 || (size_t)pos >= t.arena_n) { atomicOr(t.status, 2); continue; }
                A[pos] = (flags & T_ACC) ? A[pos] + a[idx] : a[idx];
            }
            break;
        case T_MUL:
            for (int idx = tid; idx < m * n; idx += NT) dst[idx] = a[idx] * b[idx];
            break;
        default: break;
        }
        sync();
    }
}

__global__ void __launch_bounds__(TAPE_THREADS) k_tape(TapeArgs t) {
    __shared__ double red[TAPE_THREADS];
    tape_exec<false, TAPE_THREADS>(t, t.ops, t.nops, red, nullptr, threadIdx.x);
}

// A PROGRAM over a tape: launches in order, each of them a set of record ranges ("blocks") that touch disjoint state and so
// run side by side, one workgroup per block (the updates of nodes none of which reads what another writes: the Z_n of a
// PCA-like graph, its X_n).  blocks: [first record, count] per workgroup of this launch.
__global__ void __launch_bounds__(TAPE_THREADS) k_tape_blocks(TapeArgs t, const int* blocks) {
    __shared__ double red[TAPE_THREADS];
    tape_exec<false, TAPE_THREADS>(t, t.ops + 8 * (size_t)blocks[2 * blockIdx.x], blocks[2 * blockIdx.x + 1], red, nullptr, threadIdx.x);
}

// The same with the working set in LDS: the window form of tape.h (blocks[block] = {first window, number of windows}; t.ops holds
// the resolved records).  Dynamic LDS: the window, then TAPE_CHUNK staged records.  In a BUNDLED window wavefront w interprets
// record BW b + w of bundle b on its own (tape_exec<true, 64>: no barrier inside), then the workgroup meets: a record of such a
// graph costs 300-700 ns whatever it does (profiles/tape_record_cost.py), independent ones now overlap on the SIMDs.
// BW: wavefronts of the workgroup = records of a bundle: 8 for a launch of a few long blocks, 4 for many short ones.
// tape_row: row i of a table, addressed as the table of ints it is with a 32-bit index (a 64-bit one costs k_tape_cached 100 instructions).
template <class Row> __device__ __forceinline__ const Row& tape_row(const Row* table, int i) { return *reinterpret_cast<const Row*>(reinterpret_cast<const int*>(table) + (int)(sizeof(Row) / sizeof(int)) * i); }
template <int BW>
__global__ void __launch_bounds__(64 * BW) k_tape_cached(TapeArgs t, const int* blocks, const TapeWindow* windows, const TapeSegment* segs) {
    extern __shared__ double win[];
    constexpr int NT = 64 * BW;
    __shared__ double red[NT];
    const int tid = threadIdx.x;
    const int w0 = blocks[2 * blockIdx.x], nwin = blocks[2 * blockIdx.x + 1];
    for (int w = w0; w < w0 + nwin; ++w) {
        const TapeWindow& me = tape_row(windows, w);
        const int first = me.first, count = me.count, s0 = me.seg0, ns = me.nseg, wd = me.doubles, bundled = me.bundled;
        // long segments by all threads together, short ones (most: a node's mean, a scalar) one per thread
        for (int s = 0; s < ns; ++s) {
            const TapeSegment& sg = tape_row(segs, s0 + s);
            if (sg.len < 64) continue;
            const double* src = t.arena + sg.off;
            double* dst = win + sg.lds;
            for (int idx = tid; idx < sg.len; idx += NT) dst[idx] = src[idx];
        }
        for (int s = tid; s < ns; s += NT) {
            const TapeSegment& sg = tape_row(segs, s0 + s);
            if (sg.len >= 64) continue;
            const double* src = t.arena + sg.off;
            double* dst = win + sg.lds;
            for (int idx = 0; idx < sg.len; ++idx) dst[idx] = src[idx];
        }
        int* staged = reinterpret_cast<int*>(win + ((wd + 1) & ~1));         // 16-byte aligned: records are fetched as vectors
        for (int c0 = 0; c0 < count; c0 += TAPE_CHUNK) {
            const int nc = count - c0 < TAPE_CHUNK ? count - c0 : TAPE_CHUNK;
            __syncthreads();
            const int* src = t.ops + 8 * (size_t)(first + c0);
            for (int idx = tid; idx < 8 * nc; idx += NT) staged[idx] = src[idx];
            __syncthreads();
            if (bundled) {
                for (int b0 = 0; b0 < nc; b0 += BW) {          // TAPE_CHUNK is a multiple of BW: a bundle never straddles two chunks
                    tape_exec<true, 64>(t, staged + 8 * (b0 + (tid >> 6)), 1, red, (lds_double*)win, tid & 63);
                    __syncthreads();
                }
            } else if (ns > 0) tape_exec<true, NT>(t, staged, nc, red, (lds_double*)win, tid);
            else tape_exec<false, NT>(t, staged, nc, red, nullptr, tid);
        }
        __syncthreads();
        for (int s = 0; s < ns; ++s) {
            const TapeSegment& sg = tape_row(segs, s0 + s);
            if (!sg.written || sg.len < 64) continue;
            double* dst = t.arena + sg.off;
            const double* src = win + sg.lds;
            for (int idx = tid; idx < sg.len; idx += NT) dst[idx] = src[idx];
        }
        for (int s = tid; s < ns; s += NT) {
            const TapeSegment& sg = tape_row(segs, s0 + s);
            if (!sg.written || sg.len >= 64) continue;
            double* dst = t.arena + sg.off;
            const double* src = win + sg.lds;
            for (int idx = 0; idx < sg.len; ++idx) dst[idx] = src[idx];
        }
        if (w + 1 < w0 + nwin) { __threadfence(); __syncthreads(); }        // the next window reads what this one has written back
    }
}

// ---- the host layer: handles, uploads, launches.  What a tape becomes on its way to the device is tape_plan.h's business.
struct TapeWindows {                        // the window form of a tape on the device (a TapePlan); ops null: the plain tape runs
    DeviceBuffers buf;
    int *ops = nullptr, *blocks = nullptr;
    TapeWindow* windows = nullptr; TapeSegment* segs = nullptr;
    std::vector<size_t> lds_bytes; std::vector<int> width;      // per launch
    void drop() { buf.release_all(); *this = TapeWindows(); }
};
struct Tape {
    DeviceBuffers buf;
    int* recs = nullptr; int len = 0;       // the records as given, on the device (null: destroyed) ...
    std::vector<int> host;                  // ... and on the host, for the planner
    int* blocks = nullptr;                  // program: device table {first record, count} per block, or null
    std::vector<int> launches{0, 1};        //          {first block, number of blocks} per launch (no program: the tape is one block)
    TapeWindows win;
};
struct pyvb_graph {
    int device = 0;
    bool lds_attr_set = false;              // the dynamic-LDS limit of k_tape_cached is raised on this graph's device
    hipStream_t stream = nullptr;
    DeviceBuffers buf;
    double* arena = nullptr; size_t arena_n = 0;
    int* status = nullptr;                  // bit 0: a matrix was not positive definite, bit 1: a gather / scatter index outside the arena
    std::vector<Tape> tapes;
};

// n elements at src copied into a new buffer of `buf` (an empty table: one row of zeros); a failure leaves nothing behind
template <class T> static int tape_put(DeviceBuffers& buf, T** d, const T* src, size_t n) {
    int rc = n ? buf.alloc_raw((void**)d, n * sizeof(T)) : buf.alloc((void**)d, sizeof(T));
    const hipError_t e = rc == PYVB_OK && n ? hipMemcpy(*d, src, n * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
    if (e != hipSuccess) rc = pyvb_hip_fail(e, "hipMemcpy of a tape table", __FILE__, __LINE__);
    if (rc != PYVB_OK) { buf.release(*d); *d = nullptr; }
    return rc;
}

// Plan the window form of tape `id` for the given blocks and launches and upload it.
static int tape_upload_windows(pyvb_graph* g, int id, const std::vector<int>& blocks, const std::vector<int>& launches) {
    const Tape& T = g->tapes[id];
    TapeWindows& W = g->tapes[id].win;
    W.drop();
    const TapePlan P = tape_plan(T.host, blocks, launches, g->arena_n);
    if (!P.in_lds) return PYVB_OK;
    int rc = tape_put(W.buf, &W.ops, P.cops.data(), P.cops.size());
    if (rc == PYVB_OK) rc = tape_put(W.buf, &W.blocks, P.blocks.data(), P.blocks.size());
    if (rc == PYVB_OK) rc = tape_put(W.buf, &W.windows, P.windows.data(), P.windows.size());
    if (rc == PYVB_OK) rc = tape_put(W.buf, &W.segs, P.segs.data(), P.segs.size());
    if (rc != PYVB_OK) { W.drop(); return rc; }
    W.lds_bytes = P.lds_bytes; W.width = P.width;
    return PYVB_OK;
}

extern "C" {

int pyvb_graph_create(pyvb_graph** out, int device, size_t arena_doubles) {
    ARGCHK(out && arena_doubles > 0 && arena_doubles < ((size_t)1 << 31), "bad arguments (the arena is addressed with 32-bit offsets)");
    int ndev = 0, rc;
    HIPCHK(hipGetDeviceCount(&ndev));
    ARGCHK(device >= 0 && device < ndev, "no such device");
    HIPCHK(hipSetDevice(device));
    pyvb_graph* g = new pyvb_graph();
    g->device = device; g->arena_n = arena_doubles;
    CREATE_TRYHIP(hipStreamCreate(&g->stream), pyvb_graph_destroy, g);
    CREATE_TRY(g->buf.zeros(&g->arena, arena_doubles), pyvb_graph_destroy, g);
    CREATE_TRY(g->buf.alloc((void**)&g->status, sizeof(int)), pyvb_graph_destroy, g);
    *out = g;
    return PYVB_OK;
}

int pyvb_graph_destroy(pyvb_graph* g) {
    if (!g) return PYVB_OK;
    (void)hipSetDevice(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    for (Tape& T : g->tapes) { T.buf.release_all(); T.win.drop(); }
    g->buf.release_all();
    if (g->stream) (void)hipStreamDestroy(g->stream);
    delete g;
    return PYVB_OK;
}

int pyvb_graph_write(pyvb_graph* g, size_t offset, const double* src, size_t n) {
    ARGCHK(g && src && n <= g->arena_n && offset <= g->arena_n - n, "write outside the arena");
    ENTER_DEVICE(g);
    HIPCHK(hipMemcpyAsync(g->arena + offset, src, n * sizeof(double), hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));        // src is the caller's buffer
    return PYVB_OK;
}

int pyvb_graph_sync(pyvb_graph* g) {
    ENTER_DEVICE(g);
    HIPCHK(hipStreamSynchronize(g->stream));
    int st = 0;
    HIPCHK(hipMemcpy(&st, g->status, sizeof(int), hipMemcpyDeviceToHost));
    if (st) {
        HIPCHK(hipMemset(g->status, 0, sizeof(int)));
        if (st & 2) { pyvb_set_error("a gather / scatter index of a tape pointed outside the arena (skipped)"); return PYVB_E_ARG; }
        pyvb_set_error("a posterior precision was not positive definite (numpy.linalg.LinAlgError in the reference)");
        return PYVB_E_LINALG;
    }
    return PYVB_OK;
}

int pyvb_graph_read(pyvb_graph* g, size_t offset, double* dst, size_t n) {
    ARGCHK(g && dst && n <= g->arena_n && offset <= g->arena_n - n, "read outside the arena");
    ENTER_DEVICE(g);
    HIPCHK(hipMemcpyAsync(dst, g->arena + offset, n * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    return pyvb_graph_sync(g);
}

// every extent a record touches is checked against the arena here, once, so the kernel does not have to
int pyvb_graph_tape_create(pyvb_graph* g, const int* ops, int nops, int* tape_id) {
    ARGCHK(g && ops && nops > 0 && tape_id, "bad arguments");
    for (int i = 0; i < nops; ++i) {
        if (tape_record_valid(ops + 8 * (size_t)i, g->arena_n)) continue;
        pyvb_set_error("tape record %d (opcode %d) is malformed or touches memory outside the arena", i, ops[8 * (size_t)i]);
        return PYVB_E_ARG;
    }
    ENTER_DEVICE(g);
    Tape T;
    T.len = nops; T.host.assign(ops, ops + (size_t)nops * 8);
    const int rc = tape_put(T.buf, &T.recs, ops, (size_t)nops * 8);
    if (rc != PYVB_OK) return rc;
    g->tapes.push_back(std::move(T));
    *tape_id = (int)g->tapes.size() - 1;
    return tape_upload_windows(g, *tape_id, std::vector<int>{0, nops}, g->tapes.back().launches);       // one block, one launch
}

int pyvb_graph_tape_set_program(pyvb_graph* g, int tape_id, const int* blocks, int nblocks, const int* launches, int nlaunches) {
    ARGCHK(g && tape_id >= 0 && tape_id < (int)g->tapes.size() && g->tapes[tape_id].recs, "no such tape");
    ARGCHK(blocks && launches && nblocks > 0 && nlaunches > 0, "bad arguments");
    Tape& T = g->tapes[tape_id];
    const long rec = tape_tiled(blocks, nblocks), blk = tape_tiled(launches, nlaunches);
    ARGCHK(rec >= 0, "the blocks of a program must tile the tape in order");
    ARGCHK(rec == T.len, "the blocks of a program must cover every record of the tape");
    ARGCHK(blk >= 0, "the launches of a program must tile the blocks in order");
    ARGCHK(blk == nblocks, "the launches of a program must cover every block");
    ENTER_DEVICE(g);
    HIPCHK(hipStreamSynchronize(g->stream));
    T.buf.release(T.blocks); T.blocks = nullptr;
    const int rc = tape_put(T.buf, &T.blocks, blocks, (size_t)nblocks * 2);
    if (rc != PYVB_OK) { T.win.drop(); T.launches = {0, 1}; return rc; }        // no program any more: the plain tape, one block
    T.launches.assign(launches, launches + 2 * nlaunches);
    return tape_upload_windows(g, tape_id, std::vector<int>(blocks, blocks + 2 * nblocks), T.launches);
}

int pyvb_graph_tape_run(pyvb_graph* g, int tape_id) {
    ARGCHK(g && tape_id >= 0 && tape_id < (int)g->tapes.size() && g->tapes[tape_id].recs, "no such tape");
    ENTER_DEVICE(g);
    const Tape& T = g->tapes[tape_id];
    const TapeWindows& W = T.win;
    TapeArgs t; t.arena = g->arena; t.arena_n = g->arena_n; t.ops = T.recs; t.nops = T.len; t.status = g->status;
    if (W.ops) {
        // the window form: one workgroup per block, its working set in LDS
        if (!g->lds_attr_set) {            // per graph (= per device the graph lives on; a handle is used by one host thread)
            const int cap = (int)((TAPE_LDS_CAP + 2 + TAPE_CHUNK * 4) * sizeof(double));
            HIPCHK(hipFuncSetAttribute((const void*)k_tape_cached<TAPE_BUNDLE>, hipFuncAttributeMaxDynamicSharedMemorySize, cap));
            HIPCHK(hipFuncSetAttribute((const void*)k_tape_cached<4>, hipFuncAttributeMaxDynamicSharedMemorySize, cap));
            g->lds_attr_set = true;
        }
        t.ops = W.ops;
        const std::vector<int>& L = T.launches;
        for (size_t l = 0; l + 1 < L.size(); l += 2) {
            if (W.width[l / 2] == 4)
                hipLaunchKernelGGL(k_tape_cached<4>, dim3(L[l + 1]), dim3(256), W.lds_bytes[l / 2], g->stream, t, W.blocks + 2 * L[l], W.windows, W.segs);
            else
                hipLaunchKernelGGL(k_tape_cached<TAPE_BUNDLE>, dim3(L[l + 1]), dim3(TAPE_CTHREADS), W.lds_bytes[l / 2], g->stream, t, W.blocks + 2 * L[l], W.windows, W.segs);
        }
    } else if (T.blocks) {
        for (size_t l = 0; l + 1 < T.launches.size(); l += 2)
            hipLaunchKernelGGL(k_tape_blocks, dim3(T.launches[l + 1]), dim3(TAPE_THREADS), 0, g->stream, t, T.blocks + 2 * T.launches[l]);
    } else
        hipLaunchKernelGGL(k_tape, dim3(1), dim3(TAPE_THREADS), 0, g->stream, t);
    HIPCHK(hipGetLastError());
    return PYVB_OK;
}

int pyvb_graph_tape_destroy(pyvb_graph* g, int tape_id) {
    ARGCHK(g && tape_id >= 0 && tape_id < (int)g->tapes.size(), "no such tape");
    ENTER_DEVICE(g);
    HIPCHK(hipStreamSynchronize(g->stream));
    Tape& T = g->tapes[tape_id];
    T.buf.release_all(); T.recs = T.blocks = nullptr;
    T.win.drop();
    return PYVB_OK;
}

}  // extern "C"
