// Convergence on the device (pyvb_lds_iterate_until, pyvb_lds_iterate_until_model): the stopping test of Network.learn
// (network.py:40-56, the test is on line 53) applied to the bound of a model's graph -- the sum over its chains of their six
// parts (pyvb_lds_create_tied); on a handle without tied models every replicate is its own model -- and the freeze of every
// chain of the models it stops.  The chains of a model share A, C, Q, R, so they stop together or not at all.
//   k_converge          one workgroup per replicate, right behind the k_elbo / k_elbo_dense of an iteration
// (The totals of an iteration, with the number of replicates still running, are k_elbo_sum's: k_params.hip.)
// A replicate that stops is switched off in the mask the update kernels run, exactly as pyvb_lds_set_active would: no
// update kernel loads or stores a row of it from the next launch on.  Rows of switched-off replicates sit out two ping-pongs
// (the X buffers and the covariance classes) whose positions the host tracks per handle (LdsState::x_park, cls_parked_other).
// Replicates stop in iterations of either parity, so one flag cannot say where each of them stayed: the freeze therefore
// leaves the row identical on both sides of both ping-pongs, and the flags are right for it whatever they say.
// One workgroup per replicate and not per model, so that the freeze copy of a model of many long chains is spread over as many
// workgroups as it has chains.  Every workgroup of a model therefore takes the model's decision for itself, and all of them
// must take the same one, bitwise:
//   - the bound is formed in one fixed order that depends neither on the launch nor on which chain forms it: each of the six
//     parts summed over the chains in ascending replicate order, starting from the first chain's value, then
//     ((((p0 + p1) + p2) + p3) + p4) + p5.  For a model of one chain that is the sum of the replicate's own six parts.
//   - nothing a workgroup reads is written by another in the same launch: elbo is read-only here, `old` is the workgroup's own
//     llb[n] and the run flag its own active[n].  All chains of a model hold the same values in both (they are only ever
//     written here, with the model's values, and by pyvb_lds_set_active, whose masks never split a model).
// Rows that are not the first of their model carry 0 in parts 2-5 (ParamArgs.first), in both bound modes.
#include "common.h"

struct ConvergeArgs {
    const double* elbo;         // [N][6] the parts of this iteration
    const int* mstart;          // [M + 1]: model m is replicates mstart[m] .. mstart[m + 1] - 1; null: the model of replicate n is {n}
    double* llb;                // [N] in: the model's bound of the previous test (old); out: this one
    int* iters;                 // [N]
    unsigned char* active;      // [N] the mask the update kernels run
    unsigned char* conv;        // [N]
    double tol;
    int first;                  // the first iteration of a call: old = -inf, nobody stops
    int M;
    // the freeze: current side -> other side of the X buffers and of Sigma, qld_x, lnd_x
    const double* src[4]; double* dst[4]; size_t per[4];
};

__global__ void __launch_bounds__(256) k_converge(ConvergeArgs a) {
    const int n = blockIdx.x, tid = threadIdx.x;
    // every thread takes the decision from the same values, read before thread 0 overwrites them
    const bool run = a.active[n] != 0;
    const double old = a.first ? -INFINITY : a.llb[n];
    if (!run) return;           // (the whole workgroup: a switched-off or converged model, its iters do not advance)
    int n0 = n, n1 = n + 1;
    if (a.mstart) {             // the model of this replicate: the last m with mstart[m] <= n (mstart[0] = 0, mstart[M] = N > n)
        int lo = 0, hi = a.M;
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (a.mstart[mid] <= n) lo = mid; else hi = mid;
        }
        n0 = a.mstart[lo]; n1 = a.mstart[lo + 1];
    }
    // the six parts of the model, chains in ascending order (every thread forms all of them: the loads are uniform)
    double s[6];
    for (int p = 0; p < 6; ++p) s[p] = a.elbo[(size_t)n0 * 6 + p];
    for (int c = n0 + 1; c < n1; ++c)
        for (int p = 0; p < 6; ++p) s[p] += a.elbo[(size_t)c * 6 + p];
    const double llb = ((((s[0] + s[1]) + s[2]) + s[3]) + s[4]) + s[5];
    __syncthreads();
    // network.py:53; a bound that is not finite is never convergence, a decrease is (quirk Q9)
    const bool stop = !a.first && isfinite(llb) && llb - old < a.tol;
    if (tid == 0) {
        a.llb[n] = llb;
        a.iters[n] += 1;
        if (stop) { a.conv[n] = 1; a.active[n] = 0; }
    }
    if (!stop) return;
    for (int b = 0; b < 4; ++b) {
        const double* from = a.src[b] + (size_t)n * a.per[b];
        double* d = a.dst[b] + (size_t)n * a.per[b];
        for (size_t i = tid; i < a.per[b]; i += 256) d[i] = from[i];
    }
}

int launch_converge(pyvb_lds* h, double tol, bool first, hipStream_t stream) {
    ConvergeArgs a;
    a.elbo = h->elbo; a.mstart = h->mstart; a.llb = h->conv_llb; a.iters = h->conv_iters; a.active = h->active; a.conv = h->conv;
    a.tol = tol; a.first = first ? 1 : 0; a.M = h->rep.M();
    const size_t D = h->D;
    a.src[0] = h->X[h->st.cur]; a.dst[0] = h->X[1 - h->st.cur]; a.per[0] = (size_t)h->T * h->L.DP;
    a.src[1] = h->Sigma; a.dst[1] = h->Sigma_new; a.per[1] = 3 * D * D;
    a.src[2] = h->qld_x; a.dst[2] = h->qld_x_new; a.per[2] = 3;
    a.src[3] = h->lnd_x; a.dst[3] = h->lnd_x_new; a.per[3] = 3;
    hipLaunchKernelGGL(k_converge, dim3(h->N), dim3(256), 0, stream, a);
    HIPCHK(hipGetLastError());
    return PYVB_OK;
}
