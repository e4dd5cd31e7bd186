// problem.h -- internal: the sfmba_problem handle and what the units behind include/sfmba.h need of each other
// (problem_build.hip, lm_solve.hip, sharded_solve.hip, comm_rccl.hip, sfmba_api.hip, api_frontend.hip).  Nothing here is part of the ABI.
#pragma once
#include "../../include/sfmba.h"
#include "ba_kernels.h"
#include "dense_solver.h"
#include "dist_cg.h"
#include "device_arena.h"
#include "profiler.h"
#include <algorithm>      // (the standard headers every unit behind the ABI uses)
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

struct sfmba_problem {
    int device = 0;
    int precision = SFMBA_PRECISION_F64;
    hipStream_t stream = nullptr;
    int n_cam_full = 0, n_pt_full = 0;
    int64_t n_obs = 0;
    std::vector<int> acam_id, apt_id;     // active slot -> caller index
    std::vector<int> h_pt_cnt, h_cam_cnt; // observations per point / camera slot (host mirror: CSR pointers without a device round trip)
    std::vector<int> cam_slot, pt_slot;   // caller index -> slot (-1: not observed)
    bool sharded = false;
    sfmba::DeviceStructure ds = {};
    sfmba::DeviceBuffers db = {};
    sfmba::DenseSolver solver;
    sfmba::DeviceArena arena;             // every device array below except db.trace
    sfmba::HostKit kit;                   // stream + pinned block (recycled)
    // owned device arrays behind ds
    int *d_pt_ptr = nullptr, *d_obs_cam = nullptr, *d_cam_ptr = nullptr, *d_cam_obs = nullptr, *d_cam_obs_pt = nullptr;   // (all in `arena`)
    int *d_obs_pt = nullptr, *d_perm = nullptr;   // contiguous [2*nobs]: point slot, perm
    void* d_obs_xy = nullptr;
    int4* d_chunks = nullptr, *d_chunks_coarse = nullptr, *d_pwg_desc = nullptr;
    float* d_pu32 = nullptr;                // fp32 camera records of the back-substitution's first sweep (F32J, every LM loop; launch_back_substitution)
    int2* d_pwg_chunk = nullptr; int* d_multi_slots = nullptr; int* d_build_counters = nullptr; int* d_pt_order = nullptr;
    int *d_chunk_order = nullptr, *d_coarse_order = nullptr;
    double block_fill = 1.0;              // non-empty off-diagonal blocks of the reduced matrix / all of them
    double block_band = 0.0;              // ... and the share of those that couple cameras within a quarter of the cyclic camera order
    int* d_blk_ptr = nullptr;
    unsigned* d_blk_mask = nullptr;       // per camera: cameras with a non-empty block in common (block-sparse CG product)
    int* d_cam_chunk_ptr = nullptr;
    bool deterministic = false;             // SFMBA_DETERMINISTIC=1 at build time
    bool roctx = false;                     // SFMBA_ROCTX=1 at build time: roctx ranges around the phases of an LM iteration
    bool cam_identity = false, pt_identity = false;   // slot == caller index for every camera / point (arrays copied as they are)
    bool reset_pending = false;             // sfmba_problem_reset() was called: the initial parameters are restored by the next solve's first kernel
                                            // (or by flush_reset() if anything else looks at the problem first)
    int2 *d_blk_cams = nullptr, *d_pwg_blocks = nullptr, *d_dup_blocks = nullptr;
    int* d_pair_pt = nullptr;
    void* d_cam_obs_xy = nullptr;
    double* d_facc = nullptr;
    double *d_cam0 = nullptr, *d_pts0 = nullptr;  // parameters given at create time
    double focal0 = 0.0;
    double *d_sys = nullptr;                      // S | rhs | udiag | bc (contiguous)
    double *d_red = nullptr;                      // sharded mode: packed upper triangle of S + the same tail (the all-reduce buffer)
    int* d_info = nullptr;
    sfmba::LMState* h_state = nullptr;            // pinned
    volatile int* h_lm_mail = nullptr;            // host-mapped mailbox written by k_lm_control
    char* d_pinned = nullptr;                     // device address of kit.pinned
    bool trace_mapped = false;                    // db.trace points into the pinned block
    int cur = 0;                                  // which buffer holds the current parameters
    double focal = 0.0;
    bool empty = false;                           // no observations
    bool poisoned = false;                        // an append failed half way: only sfmba_problem_destroy is valid (include/sfmba.h)
    // sharded-mode state
    sfmba_options shard_opt;
    bool shard_active = false;
    double shard_t0 = 0.0;
    int shard_rank = 0, shard_world = 1;
    double* d_scal = nullptr;                     // tail of d_sys: SFMBA_SHARD_SCALARS doubles
    int shard_host_iter = 0;
    int64_t shard_exchange[4] = { 0, 0, 0, 0 };       // bytes of exchanges (A), (B), (C) per linearisation of the last sharded solve; (B) in fp32?
    sfmba_allreduce_f32_fn allreduce_f32 = nullptr;   // optional: exchange (B) in fp32 where the CG stores S~ in fp32
    sfmba_reduce_scatter_fn reduce_scatter = nullptr; // optional: the distributed CG's exchange (B)
    // row-sharded problem (SFMBA_CREATE_ROW_SHARDED: every rank holds the whole problem; options.shard_distributed_cg = 3)
    // no pair list (SFMBA_CREATE_NO_PAIR_LIST, or more pairs of observations than a list can hold): sfmba_problem_solve runs the CG with the
    // reduced matrix applied implicitly (implicit_schur.hip) -- O(observations) memory whatever the track lengths
    bool no_pairs = false;
    bool row_sharded = false;
    int own_pt0 = 0, own_pt1 = 0, own_pt_stride = 0;  // own range of point slots; slots per rank (the per-point arrays are padded to world * stride)
    int own_chunk0 = 0, own_chunk1 = 0;               // own share of the camera-major chunks (k_cam_diag_f) ...
    int own_coarse0 = 0, own_coarse1 = 0;             // ... and of the coarse ones (column norms)
    sfmba_allgather_fn allgather = nullptr;
    sfmba::DistCg dcg;                                // distributed CG workspace (created by the first solve that asks for it)
    double *imp_dtab = nullptr, *imp_spt = nullptr, *imp_acc = nullptr, *imp_part = nullptr;   // implicit Schur product workspace (shard_distributed_cg = 2; allocated by the first solve that asks)
    long long shard_blocks_off = 0;                   // doubles: where the block region of d_red starts (behind the region of exchange (A))
    int dcg_last_f32 = -1;
    sfmba_summary shard_sum;
    sfmba::Profiler prof;
    // step probe (sfmba_problem_set_step_probe): off = no buffer, null pointers in db, nothing stored
    bool probe_on = false;
    double* d_probe = nullptr; size_t probe_cap = 0;   // [ld] z | [3 * point slots] dX (hipMalloc: it outlives the arena of an append)
    sfmba_step_probe probe = {};
};

namespace sfmba {
// the thread's last error (sfmba_last_error; sfmba_api.hip): records the message, returns rc
int fail(int rc, const std::string& msg);

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return fail(SFMBA_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)

inline double now_seconds() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Device arrays of a problem come from its arena (set for the duration of create_impl); API-call temporaries from HIP.
extern thread_local DeviceArena* t_arena;      // (problem_build.hip)
struct ArenaScope { DeviceArena* prev; explicit ArenaScope(DeviceArena* a) : prev(t_arena) { t_arena = a; } ~ArenaScope() { t_arena = prev; } };

template <typename T> hipError_t dev_alloc(T** p, size_t n) {
    if (t_arena) { *p = t_arena->alloc_n<T>(n); return *p ? hipSuccess : hipErrorOutOfMemory; }
    return hipMalloc(reinterpret_cast<void**>(p), sizeof(T) * (n ? n : 1));
}

template <typename T> hipError_t dev_upload(T** p, const std::vector<T>& v) {
    hipError_t e = dev_alloc(p, v.size());
    if (e != hipSuccess) return e;
    if (!v.empty()) e = hipMemcpy(*p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
    return e;
}
// API-call temporaries (hipMalloc: t_arena is null there), named before they are allocated: whatever they hold is freed on every return path
struct DeviceTemps {
    std::vector<void**> slots;
    template <typename... T> explicit DeviceTemps(T**... p) : slots{ reinterpret_cast<void**>(p)... } {}
    ~DeviceTemps() { for (void** s : slots) if (*s) (void)hipFree(*s); }
};

// A behaviour switch of sfmba_options: the field (1 on, -1 off), otherwise the library default.  (ABI v4 let an environment variable override
// the field; since ABI v5 nothing below sfmba_problem_create* reads the environment.)
inline bool option_switch(int field, bool dflt) { return field > 0 ? true : field < 0 ? false : dflt; }

// Calls fn(float{}) or fn(double{}) by the Jacobian precision of the handle: `with_precision(p, [&](auto t) { launch_x<decltype(t)>(...); })`
template <typename F> auto with_precision(const sfmba_problem* p, F&& fn) {
    if (p->precision == SFMBA_PRECISION_F32J) return fn(float{});
    return fn(double{});
}

int check_device(int device);
// The refusal every entry point opens with: NULL, then poisoned (a failed append), then -- where the call needs observations -- empty
int check_handle(const sfmba_problem* p, bool may_be_empty = true);
int flush_reset(sfmba_problem* p);      // the device side of sfmba_problem_reset, for the callers that are not a solve (sfmba_api.hip)

// `device` checked and current, a stream + pinned block on it for the duration of one call of an entry point without a problem handle
struct CallKit {
    HostKit kit;
    int open(int device) {
        if (const int rc = check_device(device)) return rc;
        HIP_TRY(hipSetDevice(device));
        return hostkit_acquire(device, &kit) ? SFMBA_OK : fail(SFMBA_ERR_HIP, "stream creation failed");
    }
    ~CallKit() { if (kit.stream) (void)hipStreamSynchronize(kit.stream); hostkit_release(kit); }
};

// What the passes of a ROW-SHARDED rank see (include/sfmba.h, SFMBA_CREATE_ROW_SHARDED): the point passes its own points (pt_order lists
// them), the camera-major passes its share of the chunks; everything else the whole problem.
inline DeviceStructure ds_points(const sfmba_problem* p) {
    DeviceStructure ds = p->ds;
    if (p->row_sharded) { ds.npt = p->own_pt1 - p->own_pt0; ds.pt_base = p->own_pt0; }
    return ds;
}
inline DeviceStructure ds_cams(const sfmba_problem* p) {
    DeviceStructure ds = p->ds;
    if (p->row_sharded) {
        // (a contiguous share of the LAUNCH order: the rank's workgroups stay inside one window of the point table at a time)
        ds.chunk_order += p->own_chunk0; ds.nchunk = p->own_chunk1 - p->own_chunk0;
        ds.coarse_order += p->own_coarse0; ds.nchunk_coarse = p->own_coarse1 - p->own_coarse0;
    }
    return ds;
}
}  // namespace sfmba
