// Inter-workgroup synchronisation of the persistent kernels, and the host queries that make it safe.
//
// Kernels whose workgroups wait for each other: ec_fwdp_kernel / ec_bwdp_kernel (train_ec_fwd.hip / train_fused.hip: pf_grid_barrier),
// emd_repl_kernel / emd_coop_kernel (emd.hip: pf_sum_barrier) and fps_coopm_kernel / fps_exchange_probe_kernel (patch_ops.hip:
// pf_ring_poll).  What holds them together:
//   * The HOST guarantees that THIS kernel alone fits: it launches a waiting grid only when pf_resident_per_cu (the occupancy API
//     for the kernel's block size and dynamic LDS) x the CU count covers the grid under the caller's policy.  Kernels of the same
//     process on other streams, and other processes, are not counted (FPS relies on in-order dispatch instead: the lowest
//     unfinished cloud always has all of its workgroups resident - also in a ragged launch, where clouds have different numbers
//     of workgroups: ids stay cloud-major and ascending, and a single cloud's <= 32 workgroups always fit the chip).
//   * Every wait is BOUNDED.  A waiter that runs out of budget stops waiting and its kernel reports it, so the grid drains instead
//     of hanging: ec_fwdp / ec_bwdp set the sticky word sync[3] (train_ops.check_persist_status raises), the EMD kernels make
//     their slice of dist NaN and add 1 to the status word (loss.check_emd_status), FPS writes the abort value into the cloud's
//     status word, which the other waves' polls also watch (ops._check_fps_abort).
//   * Ordering: relaxed agent-scope atomics only.  A workgroup's own global stores are complete (s_waitcnt vmcnt(0)) before its
//     arrival; there is no release / acquire fence (at agent scope a fence writes the L2 back: tens of us per barrier).
//   * A payload barrier (pf_sum_barrier) alternates TWO words by barrier parity.  A workgroup cannot reach barrier k + 2 before
//     every workgroup has arrived at k + 1, i.e. has finished polling k, so a run-ahead arrival lands in the other word and never
//     in the one a slower workgroup is still reading: every workgroup reads the same total.  With one word a workgroup that
//     passed barrier k could add its next value before a slower one had read barrier k's total (tests/test_grid_barrier_model.py).
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>
#include <vector>
#include "pf_wave.h"

// kept out of the library's dynamic symbol table.  On an inline function it also hides the function's local statics: every
// library image keeps its own copy of them
#define PF_INTERNAL __attribute__((visibility("hidden")))

// ---- arrival barrier with a generation word -----------------------------------------------------------------------------------
// Grid barrier number `gen` (1, 2, ...) of this launch: sync[0] counts arrivals, the workgroup that arrives last publishes the
// generation word sync[1] at once; sync[3] is the sticky status word (1 = a barrier timed out).  Returns false when the spin gave
// up (uniform over the workgroup).  `flag`: one int of LDS.
template <int SPIN>
__device__ __forceinline__ bool pf_grid_barrier(unsigned* sync, unsigned gen, int* flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        int fl = 0;
        if (atomicAdd(sync, 1u) == gen * gridDim.x - 1)
            PF_ST(sync + 1, gen);
        else {
            int budget = SPIN;
            while (PF_LD(sync + 1) < gen && --budget > 0) __builtin_amdgcn_s_sleep(1);
            if (budget <= 0) { fl = 2; PF_ST(sync + 3, 1u); }
        }
        *flag = fl;
    }
    __syncthreads();
    return *flag != 2;
}

// ---- arrival barrier with a payload sum -----------------------------------------------------------------------------------------
// G workgroups share `words` (two 64-bit words, zero before the launch).  At barrier nb (1, 2, ...) each adds (value << 32 | 1) to
// words[nb & 1] in ONE atomic, so the poll that sees every arrival also has the sum with it (a separate counter would cost one
// more dependent memory round trip per barrier).  Returns the sum of the G values of THIS barrier, the same in every workgroup
// (see the parity rule above); st.dead is set when the spin gave up.  The LDS state starts zeroed by the kernel.
struct PfSumBarrier {
    unsigned total;          // this barrier's sum, handed from thread 0 to the workgroup
    unsigned seen[2];        // thread 0: the running sum of each word at its previous barrier
    int dead;
};
template <int SPIN, int SLEEP>
__device__ __forceinline__ unsigned pf_sum_barrier(unsigned long long* words, unsigned nb, unsigned G, unsigned value,
                                                   PfSumBarrier& st) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long* word = words + (nb & 1);
        atomicAdd(word, ((unsigned long long)value << 32) | 1ull);
        const unsigned target = ((nb + 1) >> 1) * G;             // arrivals at the barriers of this parity so far
        int budget = SPIN;
        unsigned long long v = PF_LD(word);
        while ((unsigned)v < target && --budget > 0) {
            __builtin_amdgcn_s_sleep(SLEEP);
            v = PF_LD(word);
        }
        if (budget <= 0) st.dead = 1;
        const unsigned sum = (unsigned)(v >> 32);
        st.total = sum - st.seen[nb & 1];
        st.seen[nb & 1] = sum;
    }
    __syncthreads();
    return st.total;
}

// ---- the FPS exchange ring ------------------------------------------------------------------------------------------------------
// Wave 0's wait for one round: the `nw` words at `slot` are complete when every one carries the round's `tag` (bits 29 - 31 of the
// low half; a slot still holding the word of four rounds ago carries another tag).  Lane l reads words l, l + 64, ... into kk.
// Returns false (uniform over the wave) when the spin limit is reached or another wave has written PF_RING_ABORT into `status`.
constexpr unsigned PF_RING_SPIN = 1u << 24;
constexpr unsigned long long PF_RING_ABORT = 1ull;
template <int NT>
__device__ __forceinline__ bool pf_ring_poll(const unsigned long long* slot, int nw, unsigned tag, const unsigned long long* status,
                                             unsigned long long (&kk)[NT]) {
    const int lane = threadIdx.x & 63;
    bool dead = false;
    unsigned spins = 0;
    for (;;) {
        bool ok = true;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            kk[t] = lane + 64 * t < nw ? PF_LD(slot + lane + 64 * t) : (unsigned long long)tag;
            ok = ok && ((unsigned)kk[t] & (7u << 29)) == tag;
        }
        if (!__any(!ok)) break;
        if (++spins > PF_RING_SPIN ||
            (spins % 1024 == 0 && PF_LD(status) == PF_RING_ABORT)) {
            dead = true;
            break;
        }
    }
    return !dead;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// Dynamic LDS above 64 KiB needs hipFuncAttributeMaxDynamicSharedMemorySize on the kernel.  Set ONCE per (device, kernel) to the
// largest size any launcher of this library asks for (150 KiB: every launcher checks its own request against it), capped at what
// the device allows one workgroup beside the kernel's static LDS, behind a mutex: a per-launch set with the launch's own size let
// two host threads interleave set(small) between another thread's set(large) and its launch, cost a driver call on every launch of
// the 1 ms paths and ran inside graph captures.  Returns the HIP status; only a success is remembered.
constexpr size_t PF_LDS_CAP = 150 * 1024;
PF_INTERNAL inline hipError_t pf_allow_lds(const void* kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    static std::mutex mu;
    static std::vector<std::pair<int, const void*>> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    for (const auto& d : done)
        if (d.first == dev && d.second == kernel) return hipSuccess;
    int optin = 0;
    hipFuncAttributes fa{};
    if ((e = hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, dev)) != hipSuccess) return e;
    if ((e = hipFuncGetAttributes(&fa, kernel)) != hipSuccess) return e;
    const size_t room = (size_t)optin > fa.sharedSizeBytes ? (size_t)optin - fa.sharedSizeBytes : 0;
    const size_t want = bytes > PF_LDS_CAP ? bytes : PF_LDS_CAP;
    if ((e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(want < room ? want : room))) != hipSuccess)
        return e;
    done.emplace_back(dev, kernel);
    return hipSuccess;
}
// launchers: a failed opt-in is not remembered, and the launch that follows reports it
template <typename KERNEL>
void allow_lds(KERNEL k, size_t bytes) {
    (void)pf_allow_lds(reinterpret_cast<const void*>(k), bytes);
}

// Workgroups of `kernel` (at `threads` per workgroup and `lds` bytes of dynamic LDS) one CU of the current device can hold, and
// the device's CU count in *ncu (nullable).  0 when any query fails: "does not fit", not cached, the HIP error cleared.  Cached
// per (device, kernel, threads, LDS) behind one mutex: the queries ran on every call of the 1 ms step and inside graph captures.
PF_INTERNAL inline int pf_resident_per_cu(const void* kernel, int threads, size_t lds, int* ncu) {
    struct Entry { int dev; const void* kernel; int threads; size_t lds; int per_cu, ncu; };
    static std::mutex mu;
    static std::vector<Entry> cache;
    if (ncu) *ncu = 0;
    int dev = 0, n = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
    std::lock_guard<std::mutex> lock(mu);
    for (const auto& c : cache)
        if (c.dev == dev && c.kernel == kernel && c.threads == threads && c.lds == lds) {
            if (ncu) *ncu = c.ncu;
            return c.per_cu;
        }
    if (pf_allow_lds(kernel, lds) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    cache.push_back({dev, kernel, threads, lds, per_cu, n});
    if (ncu) *ncu = n;
    return per_cu;
}
template <typename KERNEL>
int resident_per_cu(KERNEL k, int threads, size_t lds, int* ncu) {
    return pf_resident_per_cu(reinterpret_cast<const void*>(k), threads, lds, ncu);
}
