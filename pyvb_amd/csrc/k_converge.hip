// Per-replicate convergence (pyvb_lds_iterate_until): the stopping test of Network.learn (network.py:40-56, the test is on
// line 53) applied by every replicate to its own bound, and the freeze of the replicates it stops.
//   k_converge          one workgroup per replicate, right behind the k_elbo / k_elbo_dense of an iteration
//   k_elbo_sum_running  k_elbo_sum (k_params.hip) over the mask the totals count, plus the number of replicates still running
// A replicate that stops is switched off in the mask the update kernels run, exactly as pyvb_lds_set_active would: no
// update kernel loads or stores a row of it from the next launch on.  Rows of switched-off replicates sit out two ping-pongs
// (the X buffers and the covariance classes) whose positions the host tracks per handle (LdsState::x_park, cls_parked_other).
// Replicates stop in iterations of either parity, so one flag cannot say where each of them stayed: the freeze therefore
// leaves the row identical on both sides of both ping-pongs, and the flags are right for it whatever they say.
#include "common.h"

struct ConvergeArgs {
    const double* elbo;         // [N][6] the parts of this iteration
    double* llb;                // [N] in: the bound of the previous test (old); out: this one
    int* iters;                 // [N]
    unsigned char* active;      // [N] the mask the update kernels run
    unsigned char* conv;        // [N]
    double tol;
    int first;                  // the first iteration of a call: old = -inf, nobody stops
    // the freeze: current side -> other side of the X buffers and of Sigma, qld_x, lnd_x
    const double* src[4]; double* dst[4]; size_t per[4];
};

__global__ void __launch_bounds__(256) k_converge(ConvergeArgs a) {
    const int n = blockIdx.x, tid = threadIdx.x;
    // every thread takes the decision from the same values, read before thread 0 overwrites them
    const bool run = a.active[n] != 0;
    const double* p = a.elbo + (size_t)n * 6;
    const double llb = ((((p[0] + p[1]) + p[2]) + p[3]) + p[4]) + p[5];
    const double old = a.first ? -INFINITY : a.llb[n];
    __syncthreads();
    if (!run) return;
    // network.py:53; a bound that is not finite is never convergence, a decrease is (quirk Q9)
    const bool stop = !a.first && isfinite(llb) && llb - old < a.tol;
    if (tid == 0) {
        a.llb[n] = llb;
        a.iters[n] += 1;
        if (stop) { a.conv[n] = 1; a.active[n] = 0; }
    }
    if (!stop) return;
    for (int b = 0; b < 4; ++b) {
        const double* s = a.src[b] + (size_t)n * a.per[b];
        double* d = a.dst[b] + (size_t)n * a.per[b];
        for (size_t i = tid; i < a.per[b]; i += 256) d[i] = s[i];
    }
}

// The sums of k_elbo_sum, formed in the same order, over the replicates the totals count: the running ones at their current
// bound and the converged ones at their final one.  out[6]: how many replicates are still running (it rides through the
// all-reduce with the six parts, so that every rank stops in the same iteration).
struct SumRunningArgs { const double* elbo; double* out; const unsigned char* counted; const unsigned char* active; int N; };
__global__ void __launch_bounds__(256) k_elbo_sum_running(SumRunningArgs a) {
    __shared__ double red[256 * 6];
    __shared__ int cnt[256];
    const int tid = threadIdx.x;
    double s[6] = {0, 0, 0, 0, 0, 0};
    int c = 0;
    for (int n = tid; n < a.N; n += 256) {
        if (a.counted[n])
            for (int p = 0; p < 6; ++p) s[p] += a.elbo[(size_t)n * 6 + p];
        c += a.active[n] != 0;
    }
    for (int p = 0; p < 6; ++p) red[p * 256 + tid] = s[p];
    cnt[tid] = c;
    __syncthreads();
    if (tid < 6) {
        double t = 0.0;
        for (int i = 0; i < 256; ++i) t += red[tid * 256 + i];
        a.out[tid] = t;
    } else if (tid == 6) {
        int t = 0;
        for (int i = 0; i < 256; ++i) t += cnt[i];
        a.out[6] = (double)t;
    }
}

int launch_converge(pyvb_lds* h, double tol, bool first, hipStream_t stream) {
    ConvergeArgs a;
    a.elbo = h->elbo; a.llb = h->conv_llb; a.iters = h->conv_iters; a.active = h->active; a.conv = h->conv;
    a.tol = tol; a.first = first ? 1 : 0;
    const size_t D = h->D;
    a.src[0] = h->X[h->st.cur]; a.dst[0] = h->X[1 - h->st.cur]; a.per[0] = (size_t)h->T * h->L.DP;
    a.src[1] = h->Sigma; a.dst[1] = h->Sigma_new; a.per[1] = 3 * D * D;
    a.src[2] = h->qld_x; a.dst[2] = h->qld_x_new; a.per[2] = 3;
    a.src[3] = h->lnd_x; a.dst[3] = h->lnd_x_new; a.per[3] = 3;
    hipLaunchKernelGGL(k_converge, dim3(h->N), dim3(256), 0, stream, a);
    HIPCHK(hipGetLastError());
    return PYVB_OK;
}

int launch_elbo_sum_running(pyvb_lds* h, double* out, hipStream_t stream) {
    SumRunningArgs a; a.elbo = h->elbo; a.out = out; a.counted = h->counted; a.active = h->active; a.N = h->N;
    hipLaunchKernelGGL(k_elbo_sum_running, dim3(1), dim3(256), 0, stream, a);
    HIPCHK(hipGetLastError());
    return PYVB_OK;
}
