// problem_build.hip -- sfmba_problem_create* / sfmba_problem_append / sfmba_problem_destroy: problem structure build, HBM residency.
//
// Host-side counterpart of what adjustBundle() does between BA.cpp:142 (AddResidualBlock loop) and BA.cpp:179 (ceres::Solve): the
// observation list is regrouped once per problem (point-major CSR for the point pass, camera-major CSR for the reduced-system pass)
// and uploaded.  There is NO CPU fallback: without a HIP device every entry point returns SFMBA_ERR_NO_DEVICE.
#include "problem.h"
#include "sfmba_device.h"
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>

using namespace sfmba;

thread_local DeviceArena* sfmba::t_arena = nullptr;

namespace {
// SFMBA_BUILD_TIMING: one stderr line per phase, "[sfmba <tag>] <phase> <ms since the previous mark>"
struct BuildStopwatch {
    const char* tag;
    const bool on = std::getenv("SFMBA_BUILD_TIMING") != nullptr;
    double t = now_seconds();
    void mark(const char* what) { if (on) { const double n = now_seconds(); std::fprintf(stderr, "[sfmba %s] %-18s %.3f ms\n", tag, what, 1e3 * (n - t)); t = now_seconds(); } }
};

// Host loops over the observation list of a large problem, split over a few threads (structure build of the one-shot call).
constexpr int PARALLEL_FOR_MIN = 200000;
template <typename F>
void parallel_for(int n, F fn) {
    unsigned nt = n >= PARALLEL_FOR_MIN ? std::min(8u, std::max(1u, std::thread::hardware_concurrency())) : 1u;
    if (nt <= 1) { fn(0, n); return; }
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; ++t) pool.emplace_back(fn, (int)((long long)n * t / nt), (int)((long long)n * (t + 1) / nt));
    for (auto& th : pool) th.join();
}
}  // namespace

// One resident helper thread per process: the host half of a structure build (descriptor loops, uploads) runs on it while the calling
// thread enqueues the device half.  A build takes the helper for its duration (Lease); a second build at the same time does both
// halves itself.  Never destroyed: the thread outlives static destruction.
class BuildHelper {
public:
    static BuildHelper& instance() { static BuildHelper* h = new BuildHelper(); return *h; }
    class Lease {
    public:
        explicit Lease(BuildHelper& h) : h_(h), granted_(h.alive_ && h.busy_.try_lock()) {}
        ~Lease() { if (granted_) { wait(); h_.busy_.unlock(); } }
        bool granted() const { return granted_; }
        void post(std::function<void()> fn) {
            h_.fn_ = std::move(fn);
            pending_ = true;
            h_.done_.store(false, std::memory_order_relaxed);
            h_.ready_.store(true, std::memory_order_release);
            { std::lock_guard<std::mutex> lk(h_.mu_); h_.wake_ = true; }
            h_.cv_.notify_one();
        }
        void wait() {
            if (!pending_) return;
            while (!h_.done_.load(std::memory_order_acquire)) __builtin_ia32_pause();
            pending_ = false;
        }
    private:
        BuildHelper& h_;
        bool granted_, pending_ = false;
    };
private:
    BuildHelper() {
        try { std::thread([this] { loop(); }).detach(); alive_ = true; }
        catch (...) { alive_ = false; }          // no thread to be had: every build does both halves itself
    }
    void loop() {
        for (;;) {
            { std::unique_lock<std::mutex> lk(mu_); cv_.wait(lk, [&] { return wake_; }); wake_ = false; }
            if (ready_.load(std::memory_order_acquire)) {
                ready_.store(false, std::memory_order_relaxed);
                fn_();
                fn_ = nullptr;
                done_.store(true, std::memory_order_release);
            }
        }
    }
    std::mutex busy_, mu_;
    std::condition_variable cv_;
    bool wake_ = false, alive_ = false;
    std::atomic<bool> ready_{ false }, done_{ true };
    std::function<void()> fn_;
};

extern "C" {
void sfmba_problem_destroy(sfmba_problem* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    dense_solver_destroy(&p->solver);
    if (p->d_probe) (void)hipFree(p->d_probe);
    if (p->db.trace && !p->trace_mapped) (void)hipFree(p->db.trace);
    p->arena.release();
    p->prof.destroy();
    hostkit_release(p->kit);
    delete p;
}

// Observations a (re)build starts from: the point-major arrays of the previous structure (device, old arena) and / or new
// observations on the host (caller indices, mapped through the slot tables of the problem).
struct ObsSource {
    int n_old = 0;
    const int* d_old_pt = nullptr; const int* d_old_cam = nullptr; const void* d_old_xy = nullptr; const int* d_old_perm = nullptr;
    int n_new = 0;
    const int32_t* cam = nullptr; const int32_t* pt = nullptr; const double* xy = nullptr;
};

// Builds everything that depends on the observation list into p->arena (which must be empty of structure): point-major order,
// camera-major index, pair lists, launch descriptors, parameter / record / reduced-system buffers, dense-solver workspace;
// uploads the parameters.  All sorting and list building runs on the device (structure_build.hip); the host derives the
// launch descriptors from its own per-point / per-camera observation counts (no device round trip).  The counterpart of the reference's AddResidualBlock loop
// (BA.cpp:142-166) -- and, for sfmba_problem_append, of re-running it after a view was added (SfM.cpp:464-466).
static int build_structure(sfmba_problem* p, const ObsSource& src, const double* cam6, const double* pt3, double focal, bool sharded) {
    const int device = p->device, precision = p->precision;
    BuildStopwatch bt{ "build" };
    ArenaScope arena_scope(&p->arena);
    const int ncam = (int)p->acam_id.size(), npt = (int)p->apt_id.size();
    const long long nobs64 = (long long)src.n_old + src.n_new;
    if (nobs64 >= ((long long)1 << 31)) return fail(SFMBA_ERR_INVALID_ARG, "too many observations");
    const int nobs = (int)nobs64;
    const bool f32 = precision == SFMBA_PRECISION_F32J;
    const int xy_bytes = f32 ? 8 : 16;

    // ---- per-point / per-camera observation counts on the HOST (slot order), kept across appends: the CSR pointers, the pair total
    // and every launch descriptor that depends on them are known without asking the device, so the whole structure build is one
    // enqueue with a single wait at its end (it used to be sort -> wait -> copy back -> host loop, three times over) ----
    DeviceArena staging(device);           // unsorted observations + sort temporaries: released once the stream has drained
    staging.set_zeroing(false);
    p->h_pt_cnt.resize((size_t)npt, 0); p->h_cam_cnt.resize((size_t)ncam, 0);
    // new observations as ONE packed host buffer: point slots | camera slots | caller indices | coordinates
    const size_t nn = (size_t)src.n_new;
    // (in the kit's pinned block, grown to fit and kept: the upload is a plain asynchronous copy, and a rebuild does not fault in
    // 16 MB of fresh pageable memory first -- that alone was 5 ms of the shim's rebuild path)
    const size_t h_new_bytes = (3 * sizeof(int) + (size_t)xy_bytes) * nn + 16;
    char* h_new = hostkit_upload(&p->kit, h_new_bytes);
    std::vector<char> h_new_heap(h_new ? 0 : h_new_bytes);
    if (!h_new) h_new = h_new_heap.data();
    int* h_pt = reinterpret_cast<int*>(h_new);
    int* h_cam = h_pt + nn;
    int* h_perm = h_cam + nn;
    char* h_xy = h_new + (3 * sizeof(int) * nn + 15) / 16 * 16;                  // 16-byte aligned (double2 loads on the device)
    if (src.n_new > 0) {
        const int perm0 = (int)p->n_obs - src.n_new;           // caller index of the first new observation
        std::mutex cam_mu;
        int* pt_cnt = p->h_pt_cnt.data();
        // (one thread below PARALLEL_FOR_MIN items: plain increments then -- a locked add is a full fence on x86 and would serialise the
        // cache misses of the scattered point slots, which are all this loop costs when a view is appended)
        const bool one_thread = src.n_new < PARALLEL_FOR_MIN;
        parallel_for(src.n_new, [&](int k0, int k1) {
            std::vector<int> cam_local((size_t)ncam, 0);
            for (int k = k0; k < k1; ++k) {
                if (k + 16 < k1) { const int pf = p->pt_slot[(size_t)src.pt[k + 16]]; __builtin_prefetch(pt_cnt + pf, 1); }
                const int ps = p->pt_slot[(size_t)src.pt[k]], cs = p->cam_slot[(size_t)src.cam[k]];
                h_pt[(size_t)k] = ps; h_cam[(size_t)k] = cs; h_perm[(size_t)k] = perm0 + k;
                if (one_thread) ++pt_cnt[ps]; else __atomic_fetch_add(pt_cnt + ps, 1, __ATOMIC_RELAXED);
                ++cam_local[(size_t)cs];
                if (f32) { float* d = reinterpret_cast<float*>(h_xy) + 2 * (size_t)k; d[0] = (float)src.xy[2 * (size_t)k]; d[1] = (float)src.xy[2 * (size_t)k + 1]; }
                else { double* d = reinterpret_cast<double*>(h_xy) + 2 * (size_t)k; d[0] = src.xy[2 * (size_t)k]; d[1] = src.xy[2 * (size_t)k + 1]; }
            }
            std::lock_guard<std::mutex> lk(cam_mu);
            for (int j = 0; j < ncam; ++j) p->h_cam_cnt[(size_t)j] += cam_local[(size_t)j];
        });
    }
    bt.mark("counts");
    // row-sharded: this rank's range of point slots (ceil(n / world) each: the per-point arrays are padded so that the table goes through an
    // in-place all-gather of equal slices) and its block rows of the reduced matrix (the partition of the distributed CG)
    const bool rowsh = p->row_sharded && sharded;
    int own0 = 0, own1 = npt, pt_stride = npt, brow0 = 0, brow1 = ncam;
    if (rowsh) {
        pt_stride = (npt + p->shard_world - 1) / p->shard_world;
        own0 = std::min(npt, p->shard_rank * pt_stride); own1 = std::min(npt, own0 + pt_stride);
        std::vector<int> rows; long long chunk_blocks = 0;
        dcg_partition(ncam, p->shard_world, &rows, &chunk_blocks);
        brow0 = rows[(size_t)p->shard_rank]; brow1 = rows[(size_t)p->shard_rank + 1];
    }
    p->own_pt0 = own0; p->own_pt1 = own1; p->own_pt_stride = pt_stride;
    const size_t npt_alloc = rowsh ? (size_t)pt_stride * (size_t)p->shard_world : (size_t)npt;
    PointMajor pm;
    const int64_t nblock64 = (int64_t)ncam * (ncam + 1) / 2;
    if (nblock64 >= ((int64_t)1 << 31)) return fail(SFMBA_ERR_INVALID_ARG, "too many cameras");
    const int nblock = (int)nblock64;
    auto block_of = [ncam](int ja, int jb) { return (int)((int64_t)ja * ncam - (int64_t)ja * (ja - 1) / 2 + (jb - ja)); };

    // ---- host half of the build: CSR pointers from the counts, launch descriptors, their upload, the parameters.  It runs on the
    // process's helper thread WHILE this thread enqueues the sorts (some forty launches: the enqueue is what the build costs now);
    // the two halves meet once, at the pair total (needed to size the pair list), and join before the last two launches. ----
    std::vector<int> pt_ptr((size_t)npt + 1, 0), cam_ptr((size_t)ncam + 1, 0);
    long long npair_total = 0;
    std::atomic<int> counts_state(0);            // 1 = pointers and pair total ready, -1 = counts inconsistent
    std::vector<int4> chunks, chunks_coarse;
    std::vector<int> cam_chunk_ptr((size_t)ncam + 1, 0), pt_order, chunk_order, coarse_order;
    std::vector<int2> blk_cams, pwg_blocks;
    std::vector<double> cam0, pts0;
    std::vector<char> blob;
    int pair_lpb = 64, blocks_per_wg = 1, pair_quad = 1;
    size_t pair_slot_cap = 0;
    // (SFMBA_PAIR_LIMIT: a test hook that lowers the threshold so that the matrix-free path runs at test size; read when a problem is built)
    long long pair_limit = (long long)1 << 31;
    if (const char* e = std::getenv("SFMBA_PAIR_LIMIT")) { const long long v = std::atoll(e); if (v > 0 && v < pair_limit) pair_limit = v; }
    auto host_half = [&]() -> int {
        for (int i = 0; i < npt; ++i) { const long long m = p->h_pt_cnt[(size_t)i]; pt_ptr[(size_t)i + 1] = pt_ptr[(size_t)i] + (int)m; npair_total += m * (m - 1) / 2; }
        for (int j = 0; j < ncam; ++j) cam_ptr[(size_t)j + 1] = cam_ptr[(size_t)j] + p->h_cam_cnt[(size_t)j];
        // More pairs of observations than a pair list can hold (32-bit positions; 16 bytes of sort workspace each) -- a hundred cameras that all
        // see 440k points, say; the reference adds a residual block per (view, point) without any bound on the track length, BA.cpp:142-166 --
        // or a caller that asked for it: no pair list is built and the solve applies the reduced matrix implicitly (include/sfmba.h).
        if (!sharded && npair_total >= pair_limit) p->no_pairs = true;
        const bool counts_ok = pt_ptr[(size_t)npt] == nobs && cam_ptr[(size_t)ncam] == nobs && (p->no_pairs || npair_total < ((long long)1 << 31));
        counts_state.store(counts_ok ? 1 : -1, std::memory_order_release);
        if (!counts_ok) return SFMBA_OK;         // (reported by the other half)
        // ---- launch descriptors (from the CSR pointer arrays) ----
        // chunks of the camera-major list: (camera, entry range)
        const int chunk_len = SFMBA_CAM_CHUNK;   // k_cam_diag: one lane per entry, one workgroup per chunk
        const int coarse_len = p->deterministic ? (1 << 30) : 1024;      // deterministic mode: one column-norm workgroup per camera (single writer)
        for (int j = 0; j < ncam; ++j) {
            cam_chunk_ptr[(size_t)j] = (int)chunks.size();
            for (int e0 = cam_ptr[j]; e0 < cam_ptr[(size_t)j + 1]; e0 += chunk_len) {
                int4 c; c.x = j; c.y = e0; c.z = std::min(e0 + chunk_len, cam_ptr[(size_t)j + 1]); c.w = 0;
                chunks.push_back(c);
            }
            for (int e0 = cam_ptr[j]; e0 < cam_ptr[(size_t)j + 1]; e0 += coarse_len) {
                int4 c; c.x = j; c.y = e0; c.z = (int)std::min<long long>((long long)e0 + coarse_len, cam_ptr[(size_t)j + 1]); c.w = 0;
                chunks_coarse.push_back(c);
            }
        }
        cam_chunk_ptr[(size_t)ncam] = (int)chunks.size();
        // launch order of the chunks (ba_kernels.h, chunk_order): by the chunk's relative position in its camera's list (a camera's entries ascend
        // in point slot, so that is -- for any co-visibility that samples the points evenly -- the window of the per-point table it gathers from),
        // cameras side by side inside a window (1024 windows).  The chunk list itself stays camera-major (deterministic mode adds a camera's chunks in list order).
        auto order_of = [&](const std::vector<int4>& ch, std::vector<int>* order) {
            // (a counting sort over 1024 windows, stable in list order: this runs on the append path of the incremental caller)
            constexpr int NWIN = 1024;
            order->resize(ch.size());
            std::vector<int> win(ch.size()), start(NWIN + 1, 0);
            for (size_t c = 0; c < ch.size(); ++c) {
                const int j = ch[c].x;
                const long long cnt = std::max(1, cam_ptr[(size_t)j + 1] - cam_ptr[(size_t)j]);
                const long long mid = (long long)(ch[c].y - cam_ptr[(size_t)j]) + (ch[c].z - ch[c].y) / 2;
                win[c] = (int)std::min<long long>(NWIN - 1, mid * NWIN / cnt);
                ++start[(size_t)win[c] + 1];
            }
            for (int w = 0; w < NWIN; ++w) start[(size_t)w + 1] += start[(size_t)w];
            for (size_t c = 0; c < ch.size(); ++c) (*order)[(size_t)start[(size_t)win[c]]++] = (int)c;
        };
        order_of(chunks, &chunk_order);
        order_of(chunks_coarse, &coarse_order);
        blk_cams.resize((size_t)nblock);
        for (int ja = 0; ja < ncam; ++ja)
            for (int jb = ja; jb < ncam; ++jb) { int2 c; c.x = ja; c.y = jb; blk_cams[(size_t)block_of(ja, jb)] = c; }
        // workgroups of the pair pass: consecutive blocks of ONE block-row each; rows are dealt to the 8
        // XCDs (blockIdx % 8, the observed dispatch order) so a row's records stay in one L2.  Performance
        // only: any placement gives the same result.
        // Lanes per block of the pair pass, from the mean number of pairs of an off-diagonal block: a whole wave (64 pairs per
        // round) or 16 lanes (4 blocks per wave).  Measured on MI355X: 16 lanes win at 56 pairs per block (110 vs 139 us) and
        // below (280 vs 738 us at 5.6), the whole wave wins at 226 (77 vs 105 us).  SFMBA_PAIR_LPB overrides.
        // ... per NON-EMPTY block where that is known: a handle that is rebuilt (sfmba_problem_append: the incremental loop) remembers the fill of its
        // previous structure (1.0 on the first build).  A long camera path -- 600 cameras, 6 % of the blocks non-empty, ~1 250 pairs in each of those but
        // 75 over all blocks -- runs the wave-per-chunk pass 627 -> 370 us faster than sixteen lanes per block (tools/large_banded_check.py).
        const double mean_pairs = (double)npair_total / std::max(1.0, p->block_fill * (double)std::max(1, nblock - ncam));
        pair_lpb = mean_pairs >= 128.0 ? 64 : 16;
        // A FIRST build does not know the fill.  Where the plain mean says "sixteen lanes" for a problem with many cameras, a sample decides: the
        // pairs of ~1000 points (every 2^s-th slot), their blocks sorted, m_b sampled pairs in block b -- pairs of one point never share a block, so
        // sum_b m_b (m_b - 1) estimates q^2 sum_b n_b^2 (q: the sampled share of the points) and  sum n_b^2 / sum n_b = C2 / (q * keys) + 1  is the
        // number of pairs in the block an average PAIR lives in: mean + 1 for uniform co-visibility, ~800 on the 600-camera path (mean 75).
        if (!p->no_pairs && pair_lpb == 16 && src.n_old == 0 && ncam > 64 && nn > 100000 && mean_pairs >= 8.0) {
            int shift = 0;
            while ((npt >> shift) > 1024) ++shift;
            const int mask = (1 << shift) - 1;
            std::vector<std::pair<int, int>> smp;
            { std::mutex mu;
              parallel_for((int)nn, [&](int k0, int k1) {
                  std::vector<std::pair<int, int>> loc;
                  for (int k = k0; k < k1; ++k) if ((h_pt[(size_t)k] & mask) == 0) loc.emplace_back(h_pt[(size_t)k], h_cam[(size_t)k]);
                  std::lock_guard<std::mutex> lk(mu);
                  smp.insert(smp.end(), loc.begin(), loc.end());
              }); }
            std::sort(smp.begin(), smp.end());
            std::vector<int> keys;
            size_t npts_s = 0;
            for (size_t a = 0; a < smp.size() && keys.size() < ((size_t)1 << 22);) {      // (bounded: long tracks make m (m - 1) / 2 keys per point)
                size_t b = a;
                while (b < smp.size() && smp[b].first == smp[a].first) ++b;
                ++npts_s;
                for (size_t u = a; u < b; ++u)
                    for (size_t v = u + 1; v < b; ++v) if (smp[u].second != smp[v].second) keys.push_back(block_of(std::min(smp[u].second, smp[v].second), std::max(smp[u].second, smp[v].second)));
                a = b;
            }
            std::sort(keys.begin(), keys.end());
            double c2 = 0.0;
            for (size_t a = 0; a < keys.size();) { size_t b = a; while (b < keys.size() && keys[b] == keys[a]) ++b; c2 += (double)(b - a) * (double)(b - a - 1); a = b; }
            const double q = (double)npts_s / (double)std::max(1, npt);
            const double weighted = (keys.empty() || q <= 0.0) ? mean_pairs : c2 / (q * (double)keys.size()) + 1.0;
            if (weighted >= 4.0 * 128.0) pair_lpb = 64;         // (well beyond the uniform crossover: the empty blocks of such a structure cost a wave each)
        }
        if (const char* e = std::getenv("SFMBA_PAIR_LPB")) { const int v = std::atoi(e); if (v == 64 || v == 16) pair_lpb = v; }
        blocks_per_wg = pair_lpb == 64 ? 1 : 64 / pair_lpb;
        // How the fp32 wave-per-chunk pass fetches its point-table entries: SFMBA_PAIR_LOADS=lane keeps one entry per lane (three gathers of 64 lines
        // a round), the default `quad` lets the four lanes of a quad fetch one entry per load (four loads of 16 lines, csrc/sfmba_device.h: ptrec_quad_fetch).
        // The quad form addresses the table by a 32-bit byte offset, so a table of 4 GB or more (2^26 points) keeps the per-lane loads.
        if (const char* e = std::getenv("SFMBA_PAIR_LOADS")) { if (std::strcmp(e, "lane") == 0) pair_quad = 0; }
        if ((long long)npt * 64 >= ((long long)1 << 32)) pair_quad = 0;
        {
            std::vector<std::vector<int2>> per_xcd(8);
            for (int ja = brow0; ja < (p->no_pairs ? brow0 : brow1); ++ja) {       // (a row-sharded rank: its own block rows only -- all pairs of each of their blocks; no pair list: no pair pass)
                const int b0 = block_of(ja, ja), nb = ncam - ja;
                for (int o = 0; o < nb; o += blocks_per_wg) { int2 w; w.x = b0 + o; w.y = std::min(blocks_per_wg, nb - o); per_xcd[ja % 8].push_back(w); }
            }
            size_t longest = 0;
            for (auto& v : per_xcd) longest = std::max(longest, v.size());
            for (size_t m = 0; m < longest; ++m)
                for (int x = 0; x < 8; ++x) {
                    int2 w; w.x = 0; w.y = 0;
                    if (m < per_xcd[x].size()) w = per_xcd[x][m];
                    pwg_blocks.push_back(w);
                }
        }
        // order of the points in the point passes (k_point_build / k_point_update: four lanes per point, sixteen points per
        // wave): by number of rounds of four observations, stable -- the quads of a wave then loop alike whatever the track lengths
        // (tracks of 2..30 views: a wave of unsorted points runs to its longest track).  Uniform track length: slot order, no array.
        {
            constexpr int NB = 18;                 // rounds 1 .. 16, > 16 in one bucket (+ the empty bucket 0)
            int cnt_b[NB + 1] = {};
            auto bucket = [&](int i) { const int k = pt_ptr[(size_t)i + 1] - pt_ptr[i]; return std::min((k + 3) / 4, NB - 1); };
            // (a row-sharded rank: the list of its OWN points -- always materialised, position and slot differ)
            for (int i = own0; i < own1; ++i) ++cnt_b[bucket(i) + 1];
            int used = 0;
            for (int b = 0; b < NB; ++b) used += cnt_b[b + 1] > 0;
            if (used > 1 || rowsh) {
                for (int b = 0; b < NB; ++b) cnt_b[b + 1] += cnt_b[b];
                pt_order.resize((size_t)std::max(own1 - own0, 1));
                for (int i = own0; i < own1; ++i) pt_order[(size_t)cnt_b[bucket(i)]++] = i;
            }
        }
        // upload: ONE synchronous copy on the NULL stream (the problem's stream is non-blocking: it runs beside the sorts) of the
        // arrays laid out back to back, 256-byte aligned
        {
            size_t off = 0;
            auto place = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
            const size_t o_chunks = place(sizeof(int4) * chunks.size()), o_coarse = place(sizeof(int4) * chunks_coarse.size()),
                         o_ccp = place(sizeof(int) * cam_chunk_ptr.size()), o_bc = place(sizeof(int2) * blk_cams.size()),
                         o_pwg = place(sizeof(int2) * pwg_blocks.size()), o_pto = place(sizeof(int) * pt_order.size()),
                         o_co = place(sizeof(int) * chunk_order.size()), o_cco = place(sizeof(int) * coarse_order.size());
            blob.resize(off ? off : 1);
            auto put = [&](size_t o, const void* src, size_t bytes) { if (bytes) std::memcpy(blob.data() + o, src, bytes); };
            put(o_chunks, chunks.data(), sizeof(int4) * chunks.size()); put(o_coarse, chunks_coarse.data(), sizeof(int4) * chunks_coarse.size());
            put(o_ccp, cam_chunk_ptr.data(), sizeof(int) * cam_chunk_ptr.size()); put(o_bc, blk_cams.data(), sizeof(int2) * blk_cams.size());
            put(o_pwg, pwg_blocks.data(), sizeof(int2) * pwg_blocks.size());
            put(o_pto, pt_order.data(), sizeof(int) * pt_order.size());
            put(o_co, chunk_order.data(), sizeof(int) * chunk_order.size()); put(o_cco, coarse_order.data(), sizeof(int) * coarse_order.size());
            char* d_blob = nullptr;
            HIP_TRY(dev_alloc(&d_blob, blob.size()));
            HIP_TRY(hipMemcpy(d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice));
            p->d_chunks = reinterpret_cast<int4*>(d_blob + o_chunks); p->d_chunks_coarse = reinterpret_cast<int4*>(d_blob + o_coarse);
            p->d_cam_chunk_ptr = reinterpret_cast<int*>(d_blob + o_ccp); p->d_blk_cams = reinterpret_cast<int2*>(d_blob + o_bc);
            p->d_pwg_blocks = reinterpret_cast<int2*>(d_blob + o_pwg);
            p->d_pt_order = pt_order.empty() ? nullptr : reinterpret_cast<int*>(d_blob + o_pto);
            p->d_chunk_order = reinterpret_cast<int*>(d_blob + o_co); p->d_coarse_order = reinterpret_cast<int*>(d_blob + o_cco);
        }
        // (wave-per-block pass: one descriptor per chunk of SFMBA_PAIR_CHUNK pairs -- as many as the pair total allows at most)
        pair_slot_cap = p->no_pairs ? 1 : pair_lpb == 64 ? pwg_blocks.size() + (size_t)(npair_total / SFMBA_PAIR_CHUNK) + 1 : std::max<size_t>(pwg_blocks.size() * (size_t)blocks_per_wg, 1);
        HIP_TRY(dev_alloc(&p->d_pwg_desc, pair_slot_cap));
        if (pair_lpb == 64) {
            HIP_TRY(dev_alloc(&p->d_pwg_chunk, pair_slot_cap));
            HIP_TRY(dev_alloc(&p->d_multi_slots, pwg_blocks.size() + 1));
        }
        HIP_TRY(dev_alloc(&p->d_build_counters, (size_t)4));
        HIP_TRY(dev_alloc(&p->d_dup_blocks, (size_t)ncam));
        return SFMBA_OK;
    };
    // ---- parameters.  Slot order = order of first observation; when every camera / point of the caller's arrays is observed and the slots came
    // out in index order (the usual case: point-major observation lists), the arrays go up as they are.  Runs on the helper thread behind the host
    // half (round 6: the helper had 0.24 ms to spare at BASELINE config 3 + one view while this thread enqueued; the copies are synchronous, NULL stream) ----
    auto params_half = [&]() -> int {
        bool cam_identity = (size_t)ncam == p->cam_slot.size(), pt_identity = (size_t)npt == p->pt_slot.size();
        for (int j = 0; j < ncam && cam_identity; ++j) cam_identity = p->acam_id[j] == j;
        for (int i = 0; i < npt && pt_identity; ++i) pt_identity = p->apt_id[i] == i;
        p->cam_identity = cam_identity; p->pt_identity = pt_identity;
        const double* cam_src = cam6;
        const double* pts_src = pt3;
        if (!cam_identity) {
            cam0.resize((size_t)6 * ncam);
            for (int j = 0; j < ncam; ++j) std::memcpy(&cam0[6 * (size_t)j], cam6 + 6 * (size_t)p->acam_id[j], 6 * sizeof(double));
            cam_src = cam0.data();
        }
        if (!pt_identity) {
            pts0.resize((size_t)3 * npt);
            for (int i = 0; i < npt; ++i) std::memcpy(&pts0[3 * (size_t)i], pt3 + 3 * (size_t)p->apt_id[i], 3 * sizeof(double));
            pts_src = pts0.data();
        }
        HIP_TRY(dev_alloc(&p->d_cam0, (size_t)6 * ncam));
        HIP_TRY(dev_alloc(&p->d_pts0, (size_t)3 * npt));
        if (ncam > 0) HIP_TRY(hipMemcpy(p->d_cam0, cam_src, sizeof(double) * 6 * (size_t)ncam, hipMemcpyHostToDevice));
        if (npt > 0) HIP_TRY(hipMemcpy(p->d_pts0, pts_src, sizeof(double) * 3 * (size_t)npt, hipMemcpyHostToDevice));
        return SFMBA_OK;
    };
    int host_rc = SFMBA_OK;
    std::string host_msg;
    BuildHelper::Lease helper(BuildHelper::instance());
    auto host_task = [&] {
        (void)hipSetDevice(device);
        ArenaScope helper_scope(&p->arena);
        const double th0 = now_seconds();
        host_rc = host_half();
        const double th1 = now_seconds();
        if (host_rc == SFMBA_OK && counts_state.load() > 0) host_rc = params_half();
        if (host_rc != SFMBA_OK) host_msg = sfmba_last_error();
        if (bt.on) std::fprintf(stderr, "[sfmba build] (helper) host half   %.3f ms + parameters %.3f ms\n", 1e3 * (th1 - th0), 1e3 * (now_seconds() - th1));
    };
    if (helper.granted()) helper.post(host_task); else host_task();        // (another build has the helper: everything on this thread)
    bt.mark("post");
    // ---- unsorted observations on the device: one upload of the new ones, one kernel that lays old (device to device) and new
    // ones out behind each other; then the point-major sort ----
    {
        int* u_pt = staging.alloc_n<int>((size_t)nobs);
        int* u_cam = staging.alloc_n<int>((size_t)nobs);
        int* u_perm = staging.alloc_n<int>((size_t)nobs);
        char* u_xy = static_cast<char*>(staging.alloc((size_t)xy_bytes * std::max(nobs, 1)));
        char* d_new = static_cast<char*>(staging.alloc(h_new_bytes));
        if (!u_pt || !u_cam || !u_perm || !u_xy || !d_new) { helper.wait(); return fail(SFMBA_ERR_ALLOC, "device allocation failed"); }
        hipError_t ce = hipSuccess;
        if (src.n_new > 0) ce = hipMemcpyAsync(d_new, h_new, h_new_bytes, hipMemcpyHostToDevice, p->stream);
        if (ce == hipSuccess) {
            StageObs so;
            so.n_old = src.n_old; so.n_new = src.n_new; so.old_pt = src.d_old_pt; so.old_cam = src.d_old_cam; so.old_perm = src.d_old_perm; so.old_xy = src.d_old_xy;
            so.new_pt = reinterpret_cast<const int*>(d_new); so.new_cam = so.new_pt + nn; so.new_perm = so.new_cam + nn; so.new_xy = d_new + (h_xy - h_new);
            so.u_pt = u_pt; so.u_cam = u_cam; so.u_perm = u_perm; so.u_xy = u_xy;
            launch_stage_obs(p->stream, so, xy_bytes);
            ce = hipGetLastError();
        }
        if (ce != hipSuccess) { helper.wait(); return fail(SFMBA_ERR_HIP, std::string("staging the observations: ") + hipGetErrorString(ce)); }
        bt.mark("upload obs");
        const int brc = build_point_major(p->stream, &p->arena, &staging, nobs, npt, ncam, xy_bytes, u_pt, u_cam, u_perm, u_xy, &pm);
        if (brc) { helper.wait(); return fail(SFMBA_ERR_HIP, std::string("point-major build: ") + hipGetErrorString((hipError_t)brc)); }
    }
    p->d_pt_ptr = pm.pt_ptr; p->d_obs_cam = pm.obs_cam; p->d_obs_pt = pm.obs_pt; p->d_perm = pm.obs_pt + nobs; p->d_obs_xy = pm.obs_xy;
    bt.mark("enqueue point-major");
    while (counts_state.load(std::memory_order_acquire) == 0) __builtin_ia32_pause();
    if (counts_state.load() < 0) {
        helper.wait();
        if (npair_total >= ((long long)1 << 31)) return fail(SFMBA_ERR_INVALID_ARG, "too many observation pairs for a sharded problem (2^31: the matrix-free path is unsharded)");
        return fail(SFMBA_ERR_HIP, "observation counts out of step with the observation list");
    }
    const bool no_pairs = p->no_pairs;      // (decided by the host half before it published the counts)
    // camera-pair lists: for every point, every pair of its observations (qa < qb, cameras ascending; the self pairs are folded
    // into the camera-diagonal pass) goes to block (ja, jb) of the upper triangle of S -- listed as the pair's POINT, which is all the
    // re-evaluating pair pass reads per pair
    if (no_pairs) {
        p->d_blk_ptr = p->arena.alloc_n<int>((size_t)nblock + 1);          // (all empty: the arena hands out zeroed memory)
        p->d_pair_pt = p->arena.alloc_n<int>(1);
        if (!p->d_blk_ptr || !p->d_pair_pt) { helper.wait(); return fail(SFMBA_ERR_ALLOC, "device allocation failed"); }
    } else {
        const int brc = build_pair_lists(p->stream, &p->arena, &staging, npt, nobs, ncam, nblock, p->d_pt_ptr, p->d_obs_pt, p->d_obs_cam, pm.pair_off, npair_total,
                                         &p->d_blk_ptr, &p->d_pair_pt);
        if (brc) { helper.wait(); return fail(SFMBA_ERR_HIP, std::string("pair-list build: ") + hipGetErrorString((hipError_t)brc)); }
    }
    {
        const int crc = build_camera_major(p->stream, &p->arena, &staging, nobs, ncam, p->d_obs_cam, p->d_obs_pt, &p->d_cam_obs, &p->d_cam_obs_pt, &p->d_cam_ptr);
        if (crc) { helper.wait(); return fail(SFMBA_ERR_HIP, std::string("camera-major build: ") + hipGetErrorString((hipError_t)crc)); }
    }
    {
        void* cxy = nullptr;
        const int xrc = build_camera_major_xy(p->stream, &p->arena, nobs, xy_bytes, p->d_cam_obs, p->d_obs_xy, &cxy);
        if (xrc) { helper.wait(); return fail(SFMBA_ERR_HIP, std::string("camera-major coordinates: ") + hipGetErrorString((hipError_t)xrc)); }
        p->d_cam_obs_xy = cxy;
    }
    bt.mark("enqueue sorts");
    // ---- the buffers of the solve: sized by (cameras, points, observations) alone, carved out of the arena and zeroed WHILE the helper thread finishes
    // its half (descriptors, parameters); what depends on that half -- chunk counts, the pair-pass descriptors -- follows the join ----
    DeviceStructure& ds = p->ds;
    ds = DeviceStructure{};
    ds.ncam = ncam; ds.npt = npt; ds.nobs = nobs;
    ds.d = 6 * ncam + 1;
    ds.ld = dense_padded_dim(ds.d);
    ds.nblock = nblock;          // (shard_offdiag_len below sizes the exchange buffer from it)
    DeviceBuffers& db = p->db;
    db = DeviceBuffers{};
    for (int b = 0; b < 2; ++b) {
        HIP_TRY(dev_alloc(&db.cam[b], (size_t)6 * ncam));
        HIP_TRY(dev_alloc(&db.pts[b], (size_t)3 * npt_alloc));
        HIP_TRY(dev_alloc(&db.camtab[b], (size_t)CT_STRIDE * ncam));
    }
    HIP_TRY(dev_alloc(&db.steptab, (size_t)ST_STRIDE * ncam));
    HIP_TRY(dev_alloc(&p->d_pu32, (size_t)20 * std::max(ncam, 1)));
    HIP_TRY(dev_alloc(&db.cscale, (size_t)6 * ncam));
    HIP_TRY(dev_alloc(&db.pscale, (size_t)3 * npt));
    // Nothing is stored per observation: the reduced-system passes and the back-substitution re-evaluate every observation from the
    // camera row and a per-point table (PA / PB, 64 + 24 bytes per point in fp32-Jacobian mode) plus a camera-major copy of the
    // observation coordinates (rounds 1 - 3 kept a 64-byte record per observation: 64 MB at BASELINE config 3).
    db.PA = p->arena.alloc(std::max<size_t>(npt_alloc, 1) * (f32 ? sizeof(PtRecA<float>) : sizeof(PtRecA<double>)));
    db.PB = p->arena.alloc(std::max<size_t>(npt_alloc, 1) * (f32 ? sizeof(PtRecB<float>) : sizeof(PtRecB<double>)));
    if (!db.PA || !db.PB) return fail(SFMBA_ERR_ALLOC, "device allocation failed");
    HIP_TRY(dev_alloc(&db.pt_t, (size_t)3 * npt));
    HIP_TRY(dev_alloc(&db.pt_M, (size_t)6 * npt));
    const size_t sys_len = (size_t)ds.ld * ds.ld + 3 * (size_t)ds.ld + SFMBA_SHARD_SCALARS;
    HIP_TRY(dev_alloc(&p->d_sys, sys_len));
    p->d_red = nullptr;
    if (no_pairs) {
        // the matrix-free solve runs the CG loop of the sharded path on one rank: the buffer of exchange (A)
        p->shard_blocks_off = (shard_diag_len(ds) + 63) / 64 * 64;
        HIP_TRY(dev_alloc(&p->d_red, (size_t)p->shard_blocks_off));
        p->dcg = DistCg(); p->dcg_last_f32 = -1;
        p->imp_dtab = p->imp_spt = p->imp_acc = p->imp_part = nullptr;
    }
    if (sharded) {
        // the all-reduce buffer: packed triangle of S + tail (exact solver), or the two blocks of the CG path (shard_exchange.hip, k_shard_diag)
        const size_t tri = (size_t)ds.ld * (ds.ld + 1) / 2 + 3 * (size_t)ds.ld + SFMBA_SHARD_SCALARS;
        // distributed CG: the blocks go behind the region of exchange (A), in `world` equal chunks (the padding stays zero)
        std::vector<int> rows; long long chunk = 0;
        dcg_partition(ncam, p->shard_world, &rows, &chunk);
        p->shard_blocks_off = (shard_diag_len(ds) + 63) / 64 * 64;
        const size_t dist = (size_t)p->shard_blocks_off + (size_t)p->shard_world * (size_t)chunk * 36;
        HIP_TRY(dev_alloc(&p->d_red, std::max(std::max(tri, dist), (size_t)std::max(shard_diag_len(ds), shard_offdiag_len(ds)))));
        p->dcg = DistCg(); p->dcg_last_f32 = -1;
        p->imp_dtab = p->imp_spt = p->imp_acc = p->imp_part = nullptr;
    }
    db.S = p->d_sys;
    db.rhs = db.S + (size_t)ds.ld * ds.ld;
    db.udiag = db.rhs + ds.ld;
    db.bc = db.udiag + ds.ld;
    p->d_scal = db.bc + ds.ld;
    db.shared_weight = 1.0;
    db.shard_blocks = nullptr; db.shard_blocks32 = nullptr; db.shard_scal = nullptr;
    HIP_TRY(dev_alloc(&db.st, 1));
    // padding of the reduced system (rows/columns >= d) is zero apart from the identity diagonal set by k_finalize
    HIP_TRY(hipMemsetAsync(p->d_sys, 0, sizeof(double) * sys_len, p->stream));
    HIP_TRY(dev_alloc(&p->d_info, 2));
    HIP_TRY(hipMemsetAsync(p->d_info, 0, 2 * sizeof(int), p->stream));
    db.lin_info = p->d_info;
    db.fin_counter = p->d_info + 1;
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&p->d_pinned), p->kit.pinned, 0));
    db.lm_mailbox = reinterpret_cast<int*>(p->d_pinned + 1024);
    db.st_mirror = reinterpret_cast<LMState*>(p->d_pinned);
    db.trace = nullptr; db.trace_cap = 0; p->trace_mapped = false;
    dense_solver_destroy(&p->solver);
    if (dense_solver_create(&p->solver, ds.d, ds.ld, &p->arena, p->kit.pinned + 2048)) return fail(SFMBA_ERR_ALLOC, "dense solver workspace allocation failed");
    db.pcg_bt = p->solver.vec + (size_t)8 * ds.ld;
    db.pcg_binv = p->solver.binv;
    HIP_TRY(dev_alloc(&db.pair_G, (size_t)36 * std::max(ncam, 1)));
    bt.mark("alloc buffers");
    helper.wait();
    if (host_rc != SFMBA_OK) return fail(host_rc, host_msg);
    bt.mark("join host half");
    // what depends on the block CSR is filled in by the device, behind the pair sort: the pair-pass descriptors and the list of
    // diagonal blocks that contain pairs (the same camera observing a point twice; handled by a separate pass).  The number of
    // those and the device's own pair total come back through host-mapped memory and are read after the one wait below.
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&p->d_pinned), p->kit.pinned, 0));
    volatile int* build_report = reinterpret_cast<volatile int*>(p->kit.pinned + 1536);      // [1536, 1568) of the mailbox slice
    build_report[0] = -1;
    int* d_report = reinterpret_cast<int*>(p->d_pinned + 1536);
    build_report[1] = -1; build_report[4] = -1; build_report[5] = -1; build_report[6] = -1; build_report[7] = -1;
    HIP_TRY(hipMemsetAsync(p->d_build_counters, 0, 4 * sizeof(int), p->stream));
    if (pwg_blocks.empty()) {
        build_report[4] = 0; build_report[5] = 0; build_report[7] = 0;      // (a row-sharded rank without a block row, or no pair list: no pair pass)
    } else if (pair_lpb == 64) {
        const int crc = build_pair_chunks(p->stream, &staging, (int)pwg_blocks.size(), SFMBA_PAIR_CHUNK, p->d_pwg_blocks, p->d_blk_cams, p->d_blk_ptr,
                                          p->d_pwg_desc, p->d_pwg_chunk, p->d_multi_slots, p->d_build_counters, d_report);
        if (crc) return fail(SFMBA_ERR_HIP, std::string("pair-chunk descriptors: ") + hipGetErrorString((hipError_t)crc));
    } else {
        // sixteen lanes per block: the blocks of a row grouped by rounds of sixteen pairs (a wave holds four of them and loops to the longest)
        int* d_perm = staging.alloc_n<int>((size_t)nblock);
        if (!d_perm) return fail(SFMBA_ERR_ALLOC, "device allocation failed");
        launch_row_order(p->stream, ncam, pair_lpb, p->d_blk_ptr, d_perm);
        launch_pair_desc(p->stream, (int)pwg_blocks.size(), blocks_per_wg, p->d_pwg_blocks, p->d_blk_cams, p->d_blk_ptr, d_perm, p->d_pwg_desc);
    }
    launch_block_fill(p->stream, nblock, ncam, p->d_blk_cams, p->d_blk_ptr, p->d_build_counters, d_report);
    p->d_blk_mask = nullptr;
    if (6 * ncam + 1 > 1280 && !sharded && !no_pairs) {       // (the streaming CG kernels: a sparsely filled reduced matrix is multiplied block-sparse there)
        HIP_TRY(dev_alloc(&p->d_blk_mask, (size_t)ncam * (size_t)((ncam + 31) / 32)));
        launch_block_mask(p->stream, ncam, p->d_blk_ptr, p->d_blk_mask);
    }
    launch_dup_blocks(p->stream, ncam, p->d_blk_ptr, pm.pair_off + npt, p->d_dup_blocks, d_report);
    HIP_TRY(hipGetLastError());
    p->focal0 = p->focal = focal;

    ds.pt_ptr = p->d_pt_ptr; ds.pt_order = p->d_pt_order; ds.obs_cam = p->d_obs_cam; ds.obs_xy = p->d_obs_xy;
    ds.cam_ptr = p->d_cam_ptr; ds.cam_obs = p->d_cam_obs; ds.cam_obs_pt = p->d_cam_obs_pt; ds.cam_obs_xy = p->d_cam_obs_xy;
    // row-sharded: a contiguous, equally sized share of the camera-major chunks per rank (every chunk is <= 256 entries of one camera)
    p->own_chunk0 = 0; p->own_chunk1 = (int)chunks.size(); p->own_coarse0 = 0; p->own_coarse1 = (int)chunks_coarse.size();
    if (rowsh) {
        const long long nc_ = (long long)chunks.size(), ncc = (long long)chunks_coarse.size(), r_ = p->shard_rank, w_ = p->shard_world;
        p->own_chunk0 = (int)(nc_ * r_ / w_); p->own_chunk1 = (int)(nc_ * (r_ + 1) / w_);
        p->own_coarse0 = (int)(ncc * r_ / w_); p->own_coarse1 = (int)(ncc * (r_ + 1) / w_);
    }
    ds.nchunk = (int)chunks.size(); ds.chunks = p->d_chunks; ds.chunk_order = p->d_chunk_order; ds.coarse_order = p->d_coarse_order;
    ds.nchunk_coarse = (int)chunks_coarse.size(); ds.chunks_coarse = p->d_chunks_coarse; ds.cam_chunk_ptr = p->d_cam_chunk_ptr;
    ds.obs_pt = p->d_obs_pt;
    ds.nblock = nblock; ds.blk_cams = p->d_blk_cams; ds.blk_ptr = p->d_blk_ptr; ds.pair_pt = p->d_pair_pt;
    ds.npairwg = (int)pwg_blocks.size(); ds.pwg_blocks = p->d_pwg_blocks; ds.pair_lpb = pair_lpb; ds.pair_quad = pair_quad;
    ds.pwg_group = blocks_per_wg; ds.pwg_desc = p->d_pwg_desc;
    ds.pwg_chunk = pair_lpb == 64 ? p->d_pwg_chunk : nullptr; ds.nmulti = 0; ds.multi_slots = p->d_multi_slots;      // counts: after the wait at the end
    ds.ndupwg = 0; ds.dup_blocks = p->d_dup_blocks;          // count: after the wait at the end

    // Opt-in deterministic accumulation (SFMBA_DETERMINISTIC=1 when the problem is built): every workgroup of a launch owns its
    // accumulator slot and the multi-chunk camera sums are added in chunk order, so that no result depends on the order in which
    // fp64 atomics arrive -- two runs give bit-identical trajectories.  Costs ~10 % (longer slot sweeps, a serial chunk loop).
    db.nslot = NSLOT;
    db.cd_part = nullptr;
    if (p->deterministic) {
        const int grid = std::max(std::max(1024, (ds.npt + 31) / 32 + 1), std::max(ds.nchunk, ds.nchunk_coarse));      // (point passes: 32 points per workgroup)
        db.nslot = (grid + 63) / 64 * 64;
        HIP_TRY(dev_alloc(&db.cd_part, (size_t)std::max(ds.nchunk, 1) * 48));
    }
    HIP_TRY(dev_alloc(&p->d_facc, (size_t)db.nslot * SLOT_W));
    HIP_TRY(hipMemsetAsync(p->d_facc, 0, sizeof(double) * (size_t)db.nslot * SLOT_W, p->stream));
    db.slots = p->d_facc;
    p->solver.blk_mask = p->d_blk_mask;
    bt.mark("descriptors");
    // the one wait of the build: sorts, lists and descriptors are in place; the staging arena and the host vectors may go
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (build_report[0] < 0 || (((long long)build_report[3] << 32) | (unsigned)build_report[2]) != npair_total)
        return fail(SFMBA_ERR_HIP, "structure build: the device's pair count differs from the host's");
    ds.ndupwg = no_pairs ? 0 : build_report[0];
    if (pair_lpb == 64) {
        if (build_report[4] < 0 || (size_t)build_report[4] > pair_slot_cap || build_report[5] < 0 || build_report[7] < 0 || build_report[7] > build_report[4])
            return fail(SFMBA_ERR_HIP, "structure build: pair-chunk descriptors out of range");
        ds.npairwg = build_report[4]; ds.nmulti = build_report[5];
        // partial sums: one row per chunk of the blocks that HAVE several chunks (the build counted them), not one per descriptor slot
        if (!no_pairs) HIP_TRY(dev_alloc(&db.pair_partial, (size_t)36 * std::max((int)build_report[7], 1)));
    }
    // fill of the reduced matrix: non-empty off-diagonal blocks / all of them (what SFMBA_LINEAR_AUTO reads the co-visibility from)
    p->block_fill = ncam > 1 ? (double)std::max((int)build_report[1], 0) / ((double)ncam * (ncam - 1) / 2.0) : 1.0;
    p->block_band = build_report[1] > 0 ? (double)std::max((int)build_report[6], 0) / (double)build_report[1] : 0.0;
    if (no_pairs) { p->block_fill = 1.0; p->block_band = 0.0; }      // (unknown without the list)
    p->solver.blk_fill = p->block_fill;
    bt.mark("wait for device");
    return sfmba_problem_reset(p);
}

static int create_impl(int device, int precision, int flags, int n_cam, const double* cam6, const unsigned char* cam_active, int n_pt, const double* pt3,
                       int64_t n_obs, const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_xy,
                       double focal, int rank, int world, sfmba_problem** out) {
    if (!out) return fail(SFMBA_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (n_cam < 0 || n_pt < 0 || n_obs < 0 || n_obs >= (int64_t)1 << 31) return fail(SFMBA_ERR_INVALID_ARG, "bad sizes");
    if (precision != SFMBA_PRECISION_F64 && precision != SFMBA_PRECISION_F32J) return fail(SFMBA_ERR_INVALID_ARG, "bad precision");
    if ((n_cam > 0 && !cam6) || (n_pt > 0 && !pt3) || (n_obs > 0 && (!obs_cam || !obs_pt || !obs_xy)))
        return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    int rc = check_device(device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));

    sfmba_problem* p = new sfmba_problem();
    p->device = device;
    p->arena.set_device(device);
    p->precision = precision;
    p->n_cam_full = n_cam; p->n_pt_full = n_pt; p->n_obs = n_obs;
    p->focal0 = p->focal = focal;
    p->shard_rank = rank; p->shard_world = world;
    p->no_pairs = (flags & SFMBA_CREATE_NO_PAIR_LIST) != 0;
    p->row_sharded = (flags & SFMBA_CREATE_ROW_SHARDED) != 0;
    p->sharded = cam_active != nullptr || p->row_sharded;
    // create flag, or the environment override (kept across appends: the structure is rebuilt in the same mode)
    { const char* e = std::getenv("SFMBA_DETERMINISTIC"); p->deterministic = e ? e[0] == '1' : (flags & SFMBA_CREATE_DETERMINISTIC) != 0; }
    { const char* e = std::getenv("SFMBA_ROCTX"); p->roctx = e && e[0] == '1'; }
    struct Guard { sfmba_problem* p; ~Guard() { if (p) sfmba_problem_destroy(p); } } guard{ p };

    // active (observed) cameras / points -> slots, ascending caller index
    p->cam_slot.assign((size_t)n_cam, -1); p->pt_slot.assign((size_t)n_pt, -1);
    {
        std::atomic<bool> bad(false);
        int* cs = p->cam_slot.data();
        int* ps = p->pt_slot.data();
        parallel_for((int)n_obs, [&](int k0, int k1) {
            for (int k = k0; k < k1; ++k) {
                if (obs_cam[k] < 0 || obs_cam[k] >= n_cam || obs_pt[k] < 0 || obs_pt[k] >= n_pt) { bad.store(true, std::memory_order_relaxed); return; }
                // (several threads may mark the same slot; test first: unconditional stores make the 200 camera entries' cache lines
                // bounce between the cores -- 45 ms for 10^6 observations when tried)
                if (__atomic_load_n(cs + obs_cam[k], __ATOMIC_RELAXED) != 0) __atomic_store_n(cs + obs_cam[k], 0, __ATOMIC_RELAXED);
                if (__atomic_load_n(ps + obs_pt[k], __ATOMIC_RELAXED) != 0) __atomic_store_n(ps + obs_pt[k], 0, __ATOMIC_RELAXED);
            }
        });
        if (bad.load()) return fail(SFMBA_ERR_INVALID_ARG, "observation index out of range");
    }
    if (cam_active)   // sharded: every globally observed camera is part of every rank's reduced system
        for (int j = 0; j < n_cam; ++j) if (cam_active[j]) p->cam_slot[j] = 0;
    for (int j = 0; j < n_cam; ++j) if (p->cam_slot[j] == 0) { p->cam_slot[j] = (int)p->acam_id.size(); p->acam_id.push_back(j); }
    for (int i = 0; i < n_pt; ++i) if (p->pt_slot[i] == 0) { p->pt_slot[i] = (int)p->apt_id.size(); p->apt_id.push_back(i); }
    static_assert(sizeof(LMState) <= 1024, "LMState must fit its slice of the pinned block");
    if (!hostkit_acquire(device, &p->kit)) return fail(SFMBA_ERR_HIP, "stream / pinned memory creation failed");
    p->stream = p->kit.stream;
    p->arena.set_ordering_stream(p->stream);          // zeroing of its chunks: ordered in front of the stream's work, not waited for
    p->h_state = reinterpret_cast<LMState*>(p->kit.pinned);                        // [0, 1024)
    p->h_lm_mail = reinterpret_cast<volatile int*>(p->kit.pinned + 1024);          // [1024, 1088)
    if (n_obs == 0 && !p->sharded) {
        p->empty = true;
        guard.p = nullptr;
        *out = p;
        return SFMBA_OK;
    }
    ObsSource src;
    src.n_new = (int)n_obs; src.cam = obs_cam; src.pt = obs_pt; src.xy = obs_xy;
    rc = build_structure(p, src, cam6, pt3, focal, p->sharded);
    if (rc) return rc;
    guard.p = nullptr;
    *out = p;
    return SFMBA_OK;
}

int sfmba_problem_create(int device, int precision, int n_cam, const double* cam6, int n_pt, const double* pt3,
                         int64_t n_obs, const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_xy,
                         double focal, sfmba_problem** out) {
    return create_impl(device, precision, 0, n_cam, cam6, nullptr, n_pt, pt3, n_obs, obs_cam, obs_pt, obs_xy, focal, 0, 1, out);
}

int sfmba_problem_create_ex(int device, int precision, int flags, int n_cam, const double* cam6, const unsigned char* cam_active, int n_pt,
                            const double* pt3, int64_t n_obs, const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_xy,
                            double focal, int rank, int world, sfmba_problem** out) {
    if (flags & ~(SFMBA_CREATE_DETERMINISTIC | SFMBA_CREATE_ROW_SHARDED | SFMBA_CREATE_NO_PAIR_LIST)) return fail(SFMBA_ERR_INVALID_ARG, "unknown create flag");
    if ((flags & SFMBA_CREATE_NO_PAIR_LIST) && (cam_active || (flags & SFMBA_CREATE_ROW_SHARDED))) return fail(SFMBA_ERR_INVALID_ARG, "SFMBA_CREATE_NO_PAIR_LIST applies to unsharded problems");
    const bool sharded = cam_active != nullptr || (flags & SFMBA_CREATE_ROW_SHARDED) != 0;
    if (sharded && (world < 1 || rank < 0 || rank >= world || world > SFMBA_SHARD_SCALARS - 16)) return fail(SFMBA_ERR_INVALID_ARG, "bad rank/world");
    return create_impl(device, precision, flags, n_cam, cam6, cam_active, n_pt, pt3, n_obs, obs_cam, obs_pt, obs_xy, focal,
                       sharded ? rank : 0, sharded ? world : 1, out);
}

int sfmba_problem_create_sharded(int device, int precision, int n_cam, const double* cam6, const unsigned char* cam_active,
                                 int n_pt, const double* pt3, int64_t n_obs, const int32_t* obs_cam, const int32_t* obs_pt,
                                 const double* obs_xy, double focal, int rank, int world, sfmba_problem** out) {
    if (world < 1 || rank < 0 || rank >= world || world > SFMBA_SHARD_SCALARS - 16) return fail(SFMBA_ERR_INVALID_ARG, "bad rank/world");
    return create_impl(device, precision, 0, n_cam, cam6, cam_active, n_pt, pt3, n_obs, obs_cam, obs_pt, obs_xy, focal, rank, world, out);
}

int sfmba_problem_append(sfmba_problem* p, int n_cam, const double* cam6, int n_pt, const double* pt3,
                         int64_t n_obs_new, const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_xy, double focal) {
    if (const int hrc = check_handle(p)) return hrc;
    if (p->sharded) return fail(SFMBA_ERR_INVALID_ARG, "a sharded problem cannot grow in place");
    if (p->no_pairs) return fail(SFMBA_ERR_INVALID_ARG, "a problem without a pair list cannot grow in place: create it anew");
    if (n_cam < p->n_cam_full || n_pt < p->n_pt_full || n_obs_new < 0 || p->n_obs + n_obs_new >= (int64_t)1 << 31)
        return fail(SFMBA_ERR_INVALID_ARG, "bad sizes: cameras and points can only be added at the end");
    if ((n_cam > 0 && !cam6) || (n_pt > 0 && !pt3) || (n_obs_new > 0 && (!obs_cam || !obs_pt || !obs_xy)))
        return fail(SFMBA_ERR_INVALID_ARG, "NULL array");
    HIP_TRY(hipSetDevice(p->device));
    BuildStopwatch at{ "append" };
    // (the observations of an added view are scattered over the points: the three loops over them cost their cache misses.  The
    // check pulls the slot entries in, the slot loop the counters of build_structure's loop.)
    p->cam_slot.resize((size_t)n_cam, -1); p->pt_slot.resize((size_t)n_pt, -1);
    for (int64_t k = 0; k < n_obs_new; ++k) {
        if (obs_cam[k] < 0 || obs_cam[k] >= n_cam || obs_pt[k] < 0 || obs_pt[k] >= n_pt)
            return fail(SFMBA_ERR_INVALID_ARG, "observation index out of range");
        __builtin_prefetch(&p->pt_slot[(size_t)obs_pt[k]], 1);
    }
    at.mark("check indices");
    HIP_TRY(hipStreamSynchronize(p->stream));
    at.mark("sync (idle stream)");
    // (argument errors are behind us: from here on the problem is being replaced)
    p->reset_pending = false;           // the parameters are replaced by the caller's below
    // cameras / points that become observed get the next free slot (slot order = order of first observation)
    p->h_pt_cnt.reserve((size_t)n_pt);
    for (int64_t k = 0; k < n_obs_new; ++k) {
        int& cs = p->cam_slot[(size_t)obs_cam[k]];
        if (cs < 0) { cs = (int)p->acam_id.size(); p->acam_id.push_back(obs_cam[k]); }
        int& ps = p->pt_slot[(size_t)obs_pt[k]];
        if (ps < 0) { ps = (int)p->apt_id.size(); p->apt_id.push_back(obs_pt[k]); }
        else if ((size_t)ps < p->h_pt_cnt.size()) __builtin_prefetch(&p->h_pt_cnt[(size_t)ps], 1);
    }
    p->n_cam_full = n_cam; p->n_pt_full = n_pt;
    ObsSource src;
    src.n_old = p->empty ? 0 : p->ds.nobs;
    src.d_old_pt = p->d_obs_pt; src.d_old_cam = p->d_obs_cam; src.d_old_xy = p->d_obs_xy; src.d_old_perm = p->d_perm;
    src.n_new = (int)n_obs_new; src.cam = obs_cam; src.pt = obs_pt; src.xy = obs_xy;
    p->n_obs += n_obs_new;
    if (p->n_obs == 0) { p->focal0 = p->focal = focal; return SFMBA_OK; }
    p->empty = false;
    // the new structure is built in a fresh arena (reading the old point-major arrays); the old arena then goes back to the chunk
    // cache, where the next append finds it: steady state performs no hipMalloc / hipFree
    DeviceArena old(p->device);
    old.swap(p->arena);
    if (p->db.trace && !p->trace_mapped) { (void)hipFree(p->db.trace); }
    p->db.trace = nullptr; p->db.trace_cap = 0; p->trace_mapped = false;
    p->cur = 0;
    at.mark("slots, arena swap");
    const int rc = build_structure(p, src, cam6, pt3, focal, false);
    at.mark("build_structure");
    // not failure-atomic (the old structure is gone, counts and slot tables are already the new ones): a failed build leaves the
    // handle POISONED -- every entry point refuses it from here on, only sfmba_problem_destroy is valid (include/sfmba.h)
    if (rc != SFMBA_OK) { p->poisoned = true; (void)hipStreamSynchronize(p->stream); return rc; }
    if (hipStreamSynchronize(p->stream) != hipSuccess) { p->poisoned = true; return fail(SFMBA_ERR_HIP, "structure build did not complete"); }
    at.mark("final sync");
    return rc;      // `old` releases the previous structure here
}
}  // extern "C"
