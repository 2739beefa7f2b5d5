// k_tie: several chains, one model (pyvb_lds_create_tied).  A model is a run of consecutive replicates that share the nodes
// As, Cs, Q, R; hstack, Gamma and DiagonalGamma sum over their children whoever they belong to (nodes_todo.py:43-62,
// :125-138, :183-190), so everything the parameter updates read -- the moment block of k_moments and Syy -- is the SUM over
// the chains of the model.  This kernel forms that sum once per production of what it sums and writes it into the rows of
// all the model's chains, in place: k_cols, k_resid and k_noise then run unchanged, per replicate, on identical inputs, and
// leave identical parameters in every row of the model.
//
// A deterministic segmented sum: one thread owns one element (two where the rows are 16-byte aligned) across the chains of
// its model, adds them in ascending replicate order and stores the total to every chain.  Nothing is shared between threads,
// so the result does not depend on the launch geometry.  Loads and stores are coalesced along the element index.
// Models of one chain and switched-off models leave at once (a mask never splits a model, pyvb_lds_set_active).
#include "common.h"

struct TieArgs {
    double* buf;                    // [N][per]
    const int* mstart;              // [M + 1]: model m is replicates mstart[m] .. mstart[m + 1] - 1
    const unsigned char* active;    // [N]
    size_t per;                     // doubles per replicate
    int M;
};

template <typename V>
__device__ __forceinline__ void tie_model(const TieArgs& a, int m, size_t units, size_t u) {
    const int n0 = a.mstart[m], n1 = a.mstart[m + 1];
    if (n1 - n0 < 2 || !a.active[n0]) return;
    V* row = reinterpret_cast<V*>(a.buf + (size_t)n0 * a.per) + u;
    const size_t stride = units;    // in V
    V s = row[0];
    int c = 1;
    // four loads in flight per thread: the chains of a model are a few, the latency of each load is what a thread waits for
    for (; c + 4 <= n1 - n0; c += 4) {
        const V v0 = row[(size_t)c * stride], v1 = row[(size_t)(c + 1) * stride], v2 = row[(size_t)(c + 2) * stride],
                v3 = row[(size_t)(c + 3) * stride];
        s += v0; s += v1; s += v2; s += v3;
    }
    for (; c < n1 - n0; ++c) s += row[(size_t)c * stride];
    for (c = 0; c < n1 - n0; ++c) row[(size_t)c * stride] = s;
}

template <typename V>
__global__ void __launch_bounds__(256) k_tie(TieArgs a) {
    constexpr size_t VW = sizeof(V) / sizeof(double);
    const size_t units = a.per / VW, u = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= units) return;
    for (int m = blockIdx.y; m < a.M; m += gridDim.y) tie_model<V>(a, m, units, u);     // (the grid's y extent ends at 65535)
}

// buf: h->mom (per = mom_total) or h->Syy (per = K).  Rows start 16-byte aligned exactly when per is even.
int launch_tie(pyvb_lds* h, double* buf, size_t per) {
    if (!h->mstart) return PYVB_OK;
    TieArgs a; a.buf = buf; a.mstart = h->mstart; a.active = h->active; a.per = per; a.M = h->rep.M();
    const unsigned gy = a.M < 65535 ? a.M : 65535;
    TimedLaunch tl(h, PYVB_K_PARAMS);
    if (per % 2 == 0) hipLaunchKernelGGL(k_tie<d2>, dim3((unsigned)((per / 2 + 255) / 256), gy), dim3(256), 0, h->stream, a);
    else hipLaunchKernelGGL(k_tie<double>, dim3((unsigned)((per + 255) / 256), gy), dim3(256), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    return PYVB_OK;
}
