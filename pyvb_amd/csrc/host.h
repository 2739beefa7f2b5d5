// Host-side plumbing shared by the three handle types (pyvb_lds: api.hip, pyvb_pca: api_pca.hip, pyvb_graph: k_tape.hip): argument
// and error checks, the record of the device buffers a handle owns, copies on a handle's stream.  What a pyvb_lds tracks on the
// host about what is current on the device, with the events that change it, is LdsState of lds_state.h, included here (the flow
// that decides from it which kernels a call launches is lds_flow.h).  The same for a pyvb_pca, with the planner of its sweeps, is
// pca_plan.h, included here too; a pyvb_graph keeps no such state: its tapes are planned on the host once (tape_plan.h).  What a
// handle is sized as is geometry.h.  Kernel files read the state; only the API files (through the events) write it.  DESIGN.md,
// "What is current: the host-side state of a handle", has the dependency table.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstring>
#include <vector>
#include "../../include/pyvb_hip.h"
#include "lds_state.h"
#include "pca_plan.h"

void pyvb_set_error(const char* fmt, ...);
int pyvb_hip_fail(hipError_t e, const char* what, const char* file, int line);
#define HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) return pyvb_hip_fail(_e, #x, __FILE__, __LINE__); } while (0)
#define ARGCHK(cond, msg) do { if (!(cond)) { pyvb_set_error("%s", msg); return PYVB_E_ARG; } } while (0)
// first line of an entry point: a handle, and its device current for this thread
#define ENTER_DEVICE(h) do { ARGCHK(h, "handle is NULL"); HIPCHK(hipSetDevice((h)->device)); } while (0)
// inside *_create (an int rc in scope): a failure destroys the half-built handle h with DESTROY and returns the code
#define CREATE_TRY(x, DESTROY, h) do { rc = (x); if (rc != PYVB_OK) { DESTROY(h); return rc; } } while (0)
#define CREATE_TRYHIP(x, DESTROY, h) do { hipError_t _e = (x); if (_e != hipSuccess) { rc = pyvb_hip_fail(_e, #x, __FILE__, __LINE__); DESTROY(h); return rc; } } while (0)

// Every device allocation made for a handle, recorded when it is made; *_destroy walks the record.
struct DeviceBuffers {
    std::vector<void*> owned;
    int alloc_raw(void** p, size_t bytes) {         // not filled: the caller overwrites all of it
        HIPCHK(hipMalloc(p, bytes));
        owned.push_back(*p);
        return PYVB_OK;
    }
    int alloc(void** p, size_t bytes, int fill_byte = 0) {
        const int rc = alloc_raw(p, bytes);
        if (rc != PYVB_OK) return rc;
        HIPCHK(hipMemset(*p, fill_byte, bytes));
        return PYVB_OK;
    }
    int zeros(double** p, size_t n) { return alloc((void**)p, n * sizeof(double)); }
    void release(void* p) {         // a buffer replaced during the handle's life
        for (size_t i = 0; i < owned.size(); ++i)
            if (owned[i] == p) { (void)hipFree(p); owned[i] = owned.back(); owned.pop_back(); return; }
    }
    void release_all() { for (void* p : owned) (void)hipFree(p); owned.clear(); }
};

// copies on a handle's stream; a null host pointer means "not asked for"
static inline int to_device(hipStream_t s, double* dst, const double* src, size_t n) {
    if (!src) return PYVB_OK;
    HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyHostToDevice, s));
    return PYVB_OK;
}
static inline int to_host(hipStream_t s, double* dst, const double* src, size_t n) {
    if (!dst) return PYVB_OK;
    HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost, s));
    return PYVB_OK;
}

// ---- pyvb_pca: what is current, and what the next pass over the rows is: PcaState, PcaSweepPlan and plan_sweep of pca_plan.h
