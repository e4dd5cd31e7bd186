// sharded_solve.hip -- the sharded (multi-GPU) API: the step-wise sfmba_shard_* protocol, the sharded LM loop in one call
// (sfmba_problem_solve_sharded) and the matrix-free solve of an unsharded handle without a pair list, which is that loop on one rank.
#include "lm_loop.h"
#include "sfmba_device.h"

using namespace sfmba;

extern "C" {
// ---- sharded (multi-GPU) API --------------------------------------------------------------------
// reduce_buf = [S (ld*ld) | rhs (ld) | udiag (ld) | bc (ld) | scalars]: one all-reduce(SUM) per LM iteration
// carries the partial reduced camera system, its right-hand side, the undamped diagonal, the scaled
// gradient and the linearisation scalars.  See include/sfmba.h for the protocol.
int64_t sfmba_shard_reduce_len(const sfmba_problem* p) {
    return p && !p->empty ? (int64_t)p->ds.ld * (p->ds.ld + 1) / 2 + 3 * (int64_t)p->ds.ld + SFMBA_SHARD_SCALARS : 0;
}
void* sfmba_shard_reduce_buf(sfmba_problem* p) { return p ? (void*)p->d_red : nullptr; }
int64_t sfmba_shard_setup_len(const sfmba_problem* p) { return p && !p->empty ? 2 * (int64_t)p->ds.ld + SFMBA_SHARD_SCALARS : 0; }
void* sfmba_shard_setup_buf(sfmba_problem* p) { return p ? (void*)p->db.udiag : nullptr; }
void* sfmba_shard_scalars_buf(sfmba_problem* p) { return p ? (void*)p->d_scal : nullptr; }

// fused = true (the C loop of sfmba_problem_solve_sharded, CG path): one k_begin launch carries the LM state and clears / builds what
// five launches and two copies do otherwise, and the point scales are left to the first k_point_build, as in run_solve
static int shard_begin_impl(sfmba_problem* p, const sfmba_options* opt, bool fused) {
    if (const int hrc = check_handle(p, /*may_be_empty=*/false)) return hrc;
    if (opt) p->shard_opt = *opt; else sfmba_options_default(&p->shard_opt);
    HIP_TRY(hipSetDevice(p->device));
    int rc = ensure_trace(p, std::min(std::max(p->shard_opt.max_iters, 0) + 2, 1 << 16));
    if (rc) return rc;
    if (!fused) HIP_TRY(hipStreamSynchronize(p->stream));
    p->shard_t0 = now_seconds();
    p->shard_active = true;
    p->shard_host_iter = 0;
    std::memset(&p->shard_sum, 0, sizeof(p->shard_sum));
    p->db.shared_weight = p->shard_rank == 0 ? 1.0 : 0.0;
    if ((rc = probe_arm(p))) return rc;
    LMState st;
    init_state(p, st, p->shard_opt);
    const int f32 = p->precision == SFMBA_PRECISION_F32J;
    if (p->row_sharded && !fused) return fail(SFMBA_ERR_INVALID_ARG, "a row-sharded problem runs the loop of sfmba_problem_solve_sharded only");
    if (fused) {
        *p->h_state = st;
        launch_begin(p->stream, p->ds, p->db, st, p->reset_pending ? p->d_cam0 : nullptr, p->reset_pending ? p->d_pts0 : nullptr);
        p->reset_pending = false;
        launch_xnorm(p->stream, ds_points(p), p->db);
        launch_colnorm_cams_only(p->stream, ds_cams(p), p->db, p->shard_opt.jacobi_scaling, f32, /*clear_udiag=*/false);
    } else {
        if ((rc = flush_reset(p))) return rc;
        rc = upload_state(p, st);
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(p->d_info, 0, sizeof(int), p->stream));
        launch_unit_cscale(p);
        launch_clear_slots(p->stream, p->db);
        launch_cam_setup<double>(p->stream, p->ds, p->db, p->cur);
        launch_xnorm(p->stream, p->ds, p->db);
        launch_colnorm_points_only(p->stream, p->ds, p->db, p->shard_opt.jacobi_scaling, f32);
        launch_colnorm_cams_only(p->stream, p->ds, p->db, p->shard_opt.jacobi_scaling, f32);
    }
    HIP_TRY(hipMemsetAsync(p->db.bc, 0, sizeof(double) * p->ds.ld, p->stream));
    launch_shard_pack(p->stream, p->db, p->d_scal, 0, p->shard_rank);
    return SFMBA_OK;
}
int sfmba_shard_begin(sfmba_problem* p, const sfmba_options* opt) { return shard_begin_impl(p, opt, false); }

int sfmba_shard_setup_finish(sfmba_problem* p) {
    if (!p || !p->shard_active) return fail(SFMBA_ERR_INVALID_ARG, "shard_begin was not called");
    HIP_TRY(hipSetDevice(p->device));
    launch_shard_unpack(p->stream, p->db, p->d_scal, 0, p->shard_world);
    launch_shard_xnorm_finish(p->stream, p->db);
    launch_colnorm_finish(p->stream, p->ds, p->db, p->shard_opt.jacobi_scaling);
    launch_cam_setup<double>(p->stream, p->ds, p->db, p->cur);
    return SFMBA_OK;
}

int sfmba_shard_partial_build(sfmba_problem* p) {
    if (!p || !p->shard_active) return fail(SFMBA_ERR_INVALID_ARG, "shard_begin was not called");
    HIP_TRY(hipSetDevice(p->device));
    with_precision(p, [&](auto t) { launch_partial_linearisation<decltype(t)>(p, /*ps_mode=*/0); });
    launch_cd_fold(p->stream, p->ds, p->db);       // deterministic mode: chunk sums in chunk order, before the exchange
    launch_shard_pack(p->stream, p->db, p->d_scal, 1, p->shard_rank);
    launch_shard_tri(p->stream, p->d_sys, p->d_red, p->ds.ld, 3 * (long long)p->ds.ld + SFMBA_SHARD_SCALARS, /*unpack=*/false);
    return SFMBA_OK;
}

int sfmba_shard_solve_update(sfmba_problem* p) {
    if (!p || !p->shard_active) return fail(SFMBA_ERR_INVALID_ARG, "shard_begin was not called");
    HIP_TRY(hipSetDevice(p->device));
    const sfmba_options& o = p->shard_opt;
    launch_shard_tri(p->stream, p->d_sys, p->d_red, p->ds.ld, 3 * (long long)p->ds.ld + SFMBA_SHARD_SCALARS, /*unpack=*/true);
    launch_shard_unpack(p->stream, p->db, p->d_scal, 1, p->shard_world);
    { DeviceBuffers dbf = p->db; dbf.cd_part = nullptr; launch_finalize(p->stream, p->ds, dbf, 0); }     // (chunk sums: folded before the exchange)
    DeviceBuffers dbu = p->db;
    if (p->precision == SFMBA_PRECISION_F32J) dbu.pu32 = p->d_pu32;      // (the gradient . step term is added by rank 0 only: shared_weight)
    // (AUTO's CG has no iteration cap of its own here: pcg_max_iters goes through as it is, and there is no Cholesky fallback)
    const LinearPlan plan = linear_plan(o, p->ds.d, /*always_cg=*/false, /*cap_auto_iters=*/false);
    if (plan.cg) {
        // fp32 Jacobian mode: the streaming CG path keeps the preconditioned matrix in fp32 (k_pcg_transform writes it)
        p->solver.use_f32 = p->precision == SFMBA_PRECISION_F32J && dense_pcg_want_f32(&p->solver) != nullptr;
        keep_both_triangles(p);
        // block factors and S~ from the all-reduced system, then the gauge vectors from those factors (two-level preconditioner)
        if (dense_pcg_transform(p->stream, &p->solver, p->db.S, p->db.rhs, p->d_info, nullptr)) return fail(SFMBA_ERR_ALLOC, "PCG workspace allocation failed");
        const bool coarse_cg = option_switch(o.pcg_coarse_space, true);
        if (coarse_cg) { p->db.pcg_W = p->solver.W; launch_gauge(p->stream, p->ds, p->db); }
        const int it = dense_pcg_solve(p->stream, &p->solver, p->db.S, p->db.rhs, plan.tol, plan.max_iters, p->d_info, nullptr,
                                       { .finish = false, .hist_key = p->shard_host_iter, .pretransformed = true, .anchor = plan.anchor(p->shard_host_iter == 0), .coarse = coarse_cg });
        if (it < 0) return pcg_refused(it);
        p->shard_sum.linear_iters += it;
        dbu.pcg_vec = p->solver.vec; dbu.pcg_linv = p->solver.binv; dbu.pcg_flags = p->solver.flags;
        probe_note_solver(p, true, 0);
        if (p->probe_on) p->probe.cg_iters = it;
    } else {
        dense_cholesky_solve(p->stream, &p->solver, p->db.S, p->db.rhs, p->d_info, nullptr);
        probe_note_solver(p, false, 0);
    }
    with_precision(p, [&](auto t) { launch_back_substitution<decltype(t)>(p->stream, p->ds, p->ds, dbu, nullptr); });      // (one DeviceBuffers for both: sum u . r is formed in ONE of the two)
    launch_shard_pack(p->stream, p->db, p->d_scal, 2, p->shard_rank);
    return SFMBA_OK;
}

// How an LM iteration of a sharded solve ends it: the device's verdict first, then the iteration limit (true = ended).
// (the wall-clock limit is deliberately not applied between ranks: they would disagree on it)
static bool shard_terminated(sfmba_problem* p, int termination, int message_id) {
    if (termination != -1) set_termination(p->shard_sum, termination, message_id);
    else if (p->shard_host_iter >= p->shard_opt.max_iters) set_termination(p->shard_sum, SFMBA_NO_CONVERGENCE, MSG_MAX_ITERS);
    else return false;
    return true;
}

int sfmba_shard_finish(sfmba_problem* p, int* done) {
    if (!p || !p->shard_active || !done) return fail(SFMBA_ERR_INVALID_ARG, "shard_begin was not called");
    HIP_TRY(hipSetDevice(p->device));
    launch_shard_unpack(p->stream, p->db, p->d_scal, 2, p->shard_world);
    launch_control(p->stream, p->ds, p->db);
    if (const int rc = download_state(p)) return rc;
    p->shard_host_iter = p->h_state->iter;
    *done = shard_terminated(p, p->h_state->termination, p->h_state->message) ? 1 : 0;
    return SFMBA_OK;
}

int sfmba_shard_end(sfmba_problem* p, sfmba_summary* summary) {
    if (!p || !p->shard_active) return fail(SFMBA_ERR_INVALID_ARG, "shard_begin was not called");
    HIP_TRY(hipSetDevice(p->device));
    int rc = download_state(p);
    if (rc) return rc;
    p->db.shared_weight = 1.0;
    p->shard_active = false;
    sfmba_summary& sum = p->shard_sum;
    fill_summary(p, sum, p->shard_t0);
    TraceRow row0;
    if ((rc = read_trace_rows(p, &row0, 1))) return rc;
    sum.initial_cost = row0.cost;
    if (summary) *summary = sum;
    return SFMBA_OK;
}

// ---- the sharded LM loop in one call: collectives through a callback (RCCL in comm_rccl.hip, or the caller's) ----
static int solve_sharded_impl(sfmba_problem* p, const sfmba_options* opt, sfmba_allreduce_fn allreduce, void* ctx, sfmba_summary* summary) {
    if (p->shard_world > 1 && !allreduce) return fail(SFMBA_ERR_INVALID_ARG, "world > 1 needs an all-reduce");
    const double t_shard0 = now_seconds();
    auto collective = [](int crc, const char* what) { return crc == 0 ? SFMBA_OK : fail(SFMBA_ERR_HIP, std::string(what) + " failed (rc " + std::to_string(crc) + ")"); };
    // (a communicator of one rank is still called: the RCCL path is exercised on a one-GPU box)
    auto reduce = [&](void* buf, int64_t n) { return allreduce ? collective(allreduce(ctx, buf, n, (void*)p->stream), "all-reduce") : SFMBA_OK; };
    sfmba_options o_in;
    if (opt) o_in = *opt; else sfmba_options_default(&o_in);
    // (a row-sharded problem: always the CG loop -- a rank holds all observations, the single all-reduce of partial systems does not apply)
    const bool two_phase = p->row_sharded || p->no_pairs || (linear_plan(o_in, p->ds.d, /*always_cg=*/false, /*cap_auto_iters=*/false).cg &&
                                                             option_switch(o_in.shard_two_phase, true));
    if (p->row_sharded && p->shard_world > 1 && !p->allgather) return fail(SFMBA_ERR_INVALID_ARG, "a row-sharded solve with world > 1 needs sfmba_problem_set_allgather");
    // fail-stop rule (include/sfmba.h): everything the loop allocates is allocated before this rank's first collective
    if (two_phase) {
        if (dense_pcg_ensure_workspace(&p->solver)) return fail(SFMBA_ERR_ALLOC, "PCG workspace allocation failed");
        if (p->precision == SFMBA_PRECISION_F32J) (void)dense_pcg_want_f32(&p->solver);     // (null = not applicable at this size)
    }
    int rc = shard_begin_impl(p, opt, /*fused=*/two_phase);
    if (rc) return rc;
    p->h_lm_mail[0] = 0; p->h_lm_mail[1] = -1;
    if ((rc = reduce(sfmba_shard_setup_buf(p), sfmba_shard_setup_len(p)))) return rc;
    if ((rc = sfmba_shard_setup_finish(p))) return rc;
    const sfmba_options& o = p->shard_opt;
    int controls = 0;
    if (two_phase) {
        // CG solver: two all-reduces per linearisation (diagonal blocks + vectors, then the off-diagonal blocks of the preconditioned
        // matrix, shard_exchange.hip k_shard_diag / k_shard_offdiag) and the same fused kernels as the one-GPU loop in run_solve:
        // block factors and gauge vectors in k_finalize, transform in the pair pass, gated CG batches (no host wait on the solve).
        const bool coarse_cg = option_switch(o.pcg_coarse_space, true);
        const bool f32 = p->precision == SFMBA_PRECISION_F32J;
        bool first_linear_solve = true;
        const bool speculate = option_switch(o.early_linearise, true);
        bool build_enqueued = false;
        const bool exchange_f32_off = !option_switch(o.shard_f32_exchange, true);
        // AUTO here = the CG run to a plain relative 1e-12 (no Cholesky fallback in the sharded loop: the factorisation would need the
        // unpreconditioned matrix exchanged as well; at max_iters the step is forced, as with PCG).  This loop also serves row-sharded and
        // matrix-free handles whose options say Cholesky: everything that is not SFMBA_LINEAR_PCG is the exact CG; pcg_max_iters goes through as it is.
        const LinearPlan plan = linear_plan(o, p->ds.d, /*always_cg=*/true, /*cap_auto_iters=*/false);
        const double cg_tol = plan.tol;
        // the CG without the redundant solve (dist_cg.h): reduce-scatter of the blocks, products from the owned blocks, one small
        // all-reduce per CG iteration
        // ... or WITHOUT any exchange of the reduced matrix (shard_distributed_cg = 2): the product of a CG iteration is formed implicitly from
        // every rank's own points (implicit_schur.hip)
        int dist_mode = o.shard_distributed_cg > 0 ? o.shard_distributed_cg : 0;
        // ... or with the block ROWS of S~ sharded (shard_distributed_cg = 3): a property of the problem handle -- every rank was given the whole problem
        if (p->no_pairs) dist_mode = 2;          // no pair list: the implicit product is the only one there is
        else if (p->row_sharded) dist_mode = 3;
        else if (dist_mode == 3) return fail(SFMBA_ERR_INVALID_ARG, "shard_distributed_cg = 3 needs a problem created with SFMBA_CREATE_ROW_SHARDED");
        // (duplicate (camera, point) observations: the implicit product sums over ALL pairs of a point's observations, those of one camera
        // included, so in that form their cross terms are simply not added to the diagonal blocks -- which stay what they are for: a
        // preconditioner.  Nothing is decided from a rank's own duplicate count: every rank takes the form the options name)
        const bool implicit_cg = dist_mode == 2;
        const bool row_cg = dist_mode == 3;
        const bool dist_cg = dist_mode > 0 && (implicit_cg || row_cg || p->shard_world == 1 || p->reduce_scatter != nullptr);
        const DeviceStructure dsp = ds_points(p), dsc = ds_cams(p);
        const size_t pa_bytes = f32 ? sizeof(PtRecA<float>) : sizeof(PtRecA<double>), pb_bytes = f32 ? sizeof(PtRecB<float>) : sizeof(PtRecB<double>);
        // (one rank; a communicator of one rank is still called)
        auto gather = [&](void* buf, size_t bytes_per_rank) { return p->allgather ? collective(p->allgather(ctx, buf, (int64_t)bytes_per_rank, (void*)p->stream), "all-gather") : SFMBA_OK; };
        struct ArCtx { sfmba_allreduce_fn fn; void* ctx; } arctx{ allreduce, ctx };
        auto ar_thunk = [](void* c, void* buf, long long n, hipStream_t st) -> int { ArCtx* a = static_cast<ArCtx*>(c); return a->fn ? a->fn(a->ctx, buf, (int64_t)n, (void*)st) : 0; };
        int dcg_launched = 0, dcg_max = o.pcg_max_iters > 0 ? o.pcg_max_iters : 4 * p->ds.d;
        if (dist_cg && !p->dcg.ready) {
            ArenaScope as(&p->arena);
            if (dcg_create(&p->dcg, p->ds.d, p->ds.ld, p->ds.ncam, p->shard_rank, p->shard_world, &p->arena)) return fail(SFMBA_ERR_ALLOC, "distributed CG workspace allocation failed");
        }
        if (implicit_cg && !p->imp_dtab) {
            ArenaScope as(&p->arena);
            p->imp_dtab = p->arena.alloc_n<double>((size_t)8 * std::max(p->ds.ncam, 1));
            p->imp_spt = p->arena.alloc_n<double>((size_t)3 * std::max(p->ds.npt, 1));
            p->imp_acc = p->arena.alloc_n<double>((size_t)6 * std::max(p->ds.ncam, 1));
            if (p->deterministic) p->imp_part = p->arena.alloc_n<double>((size_t)6 * std::max(p->ds.nchunk, 1));
            if (!p->imp_dtab || !p->imp_spt || !p->imp_acc || (p->deterministic && !p->imp_part)) { p->imp_dtab = nullptr; return fail(SFMBA_ERR_ALLOC, "implicit Schur workspace allocation failed"); }
        }
        ImplicitProduct ip;
        int first_build = o.jacobi_scaling ? 1 : 2;          // the first point pass also forms the point scales
        bool limit_exit = false;         // the loop ended on the iteration or time limit, not by the device's verdict
        for (;;) {
            if (dense_pcg_ensure_workspace(&p->solver)) return fail(SFMBA_ERR_ALLOC, "PCG workspace allocation failed");
            p->db.pcg_F = p->solver.Sfull;
            p->db.pcg_W = coarse_cg ? p->solver.W : nullptr;
            float* F32 = (f32 && !implicit_cg) ? dense_pcg_want_f32(&p->solver) : nullptr;      // (implicit product: there is no matrix to store)
            p->solver.use_f32 = F32 != nullptr;
            keep_both_triangles(p);      // (of the replicated matrix)
            // the streaming CG path stores S~ in fp32: with a single-precision all-reduce the partial blocks are exchanged in fp32 and
            // the sum is the CG's matrix (what the camera pass and the pair epilogue write directly -- diagonal blocks, focal column --
            // goes to the fp32 matrix as on one GPU); otherwise everything is summed in fp64 and narrowed after the sum
            // (one rank without a communicator: nothing is exchanged, the blocks stay in the CG's own precision)
            const bool x32 = F32 != nullptr && !exchange_f32_off && (row_cg || (p->allreduce_f32 != nullptr && allreduce != nullptr) || (p->shard_world == 1 && allreduce == nullptr));
            p->db.pcg_F32 = x32 ? F32 : nullptr;
            p->shard_exchange[0] = 8 * shard_diag_len(p->ds); p->shard_exchange[1] = (x32 ? 4 : 8) * shard_offdiag_len(p->ds);
            p->shard_exchange[2] = 8 * SFMBA_SHARD_SCALARS; p->shard_exchange[3] = x32 ? 1 : 0;
            if (!build_enqueued) with_precision(p, [&](auto t) { launch_point_build<decltype(t)>(p->stream, dsp, p->db, first_build); });
            build_enqueued = false;
            if (row_cg) {
                // the per-point table of every rank's points: what the camera pass and the pair pass re-evaluate the observations from
                if ((rc = gather(p->db.PA, (size_t)p->own_pt_stride * pa_bytes))) return rc;
                if ((rc = gather(p->db.PB, (size_t)p->own_pt_stride * pb_bytes))) return rc;
            }
            // (deterministic mode: a chunk's slot in cd_part is its index in the chunk LIST, whatever the launch order; the slots of the others' chunks stay zero)
            with_precision(p, [&](auto t) { launch_cam_diag<decltype(t)>(p->stream, dsc, p->db); });
            // pairs inside diagonal blocks: part of the implicit product; a row-sharded rank holds ALL of them -- rank 0 adds them
            if (!implicit_cg && (!row_cg || p->shard_rank == 0)) with_precision(p, [&](auto t) { launch_schur_pairs<decltype(t)>(p->stream, p->ds, p->db, 2); });
            first_build = 0;
            launch_cd_fold(p->stream, p->ds, p->db);       // deterministic mode: chunk sums in chunk order, before the exchange
            launch_shard_diag(p->stream, p->ds, p->db, p->d_red, /*unpack=*/false, p->shard_rank, p->shard_world);
            if ((rc = reduce(p->d_red, shard_diag_len(p->ds)))) return rc;
            launch_shard_diag(p->stream, p->ds, p->db, p->d_red, /*unpack=*/true, p->shard_rank, p->shard_world);
            { DeviceBuffers dbf = p->db; dbf.cd_part = nullptr; launch_finalize(p->stream, p->ds, dbf, 1); }
            // the pair pass stores its transformed blocks straight into the all-reduce buffer
            DcgSolveArgs da;
            if (dist_cg) {
              const int fo = p->ds.d - 1;
              if (implicit_cg) {
                // no pair pass, no exchange (B): the glue the pair pass does on the way (focal row of S~, b~, post-linearisation) on its own
                launch_pcg_glue(p->stream, p->ds, p->db);
                ip.ds = p->ds; ip.db = p->db; ip.dtab = p->imp_dtab; ip.spt = p->imp_spt; ip.acc = p->imp_acc; ip.part = p->imp_part;
                ip.focal_row = p->solver.Sfull + (size_t)fo * p->ds.ld; ip.focal_row32 = nullptr; ip.rank = p->shard_rank; ip.f32 = f32;
                da.implicit = &ip;
                p->shard_exchange[1] = 0; p->shard_exchange[3] = 2 | 4;
              } else {
                // row-sharded: the glue for ALL cameras on its own (the pair pass below only visits the diagonal blocks of the rank's rows)
                if (row_cg) launch_pcg_glue(p->stream, p->ds, p->db);
                // ... in the reduce-scatter layout (`world` equal chunks of whole block rows behind the region of exchange (A); padding zero)
                double* blocks = p->d_red + p->shard_blocks_off;
                const long long cv = dcg_chunk_values(p->dcg), total = cv * p->shard_world;
                if (p->dcg_last_f32 != (x32 ? 1 : 0)) { HIP_TRY(hipMemsetAsync(blocks, 0, (size_t)total * (x32 ? 4 : 8), p->stream)); p->dcg_last_f32 = x32 ? 1 : 0; }
                p->db.shard_row_shift = p->dcg.d_row_shift;
                if (x32) p->db.shard_blocks32 = reinterpret_cast<float*>(blocks); else p->db.shard_blocks = blocks;
                with_precision(p, [&](auto t) { launch_schur_pairs<decltype(t)>(p->stream, p->ds, p->db, 1); });
                p->db.shard_blocks = nullptr; p->db.shard_blocks32 = nullptr; p->db.shard_row_shift = nullptr;
                char* mine = reinterpret_cast<char*>(blocks) + (size_t)p->shard_rank * (size_t)cv * (x32 ? 4 : 8);
                if (p->shard_world > 1 && !row_cg) {
                    if ((rc = collective(p->reduce_scatter(ctx, blocks, mine, (int64_t)cv, x32 ? 1 : 0, (void*)p->stream), "reduce-scatter"))) return rc;
                }
                p->shard_exchange[1] = (x32 ? 4 : 8) * total; p->shard_exchange[3] = (x32 ? 1 : 0) | 2;
                // (row-sharded: the rank's blocks are complete as they leave the pair pass -- what crosses the ranks is the per-point table)
                if (row_cg) { p->shard_exchange[1] = (long long)(p->shard_world - 1) * p->own_pt_stride * (long long)(pa_bytes + pb_bytes); p->shard_exchange[3] = (x32 ? 1 : 0) | 2 | 8; }
                da.owned = mine; da.owned_f32 = x32;
                if (p->db.pcg_F32) da.focal_row32 = p->db.pcg_F32 + (size_t)fo * p->ds.ld; else da.focal_row = p->solver.Sfull + (size_t)fo * p->ds.ld;
              }
                da.bt = p->solver.vec + (size_t)8 * p->ds.ld; da.W = coarse_cg ? p->solver.W : nullptr;
                da.flags = p->solver.flags; da.info = p->d_info; da.tol = cg_tol;
                da.anchor = plan.anchor(first_linear_solve);
                { const double t2 = cg_tol * cg_tol; da.cap = t2 > 0.0 ? std::max(t2, 1e-8) / t2 : 1.0; }
                first_linear_solve = false;
                p->dcg.x = p->solver.vec;
                int drc = dcg_begin(p->stream, &p->dcg, da, ar_thunk, &arctx);
                int batch = 24;
                // (every launch of a batch issues its collective, converged or not: one launch in reserve, not two -- a surplus iteration is a whole
                // all-reduce at N > 1; a batch one short costs one host round trip)
                if (p->shard_host_iter < (int)p->solver.hist.size() && p->solver.hist[(size_t)p->shard_host_iter] > 0) batch = p->solver.hist[(size_t)p->shard_host_iter] + 1;
                batch = std::min(batch, dcg_max);
                if (!drc) drc = dcg_iterate(p->stream, &p->dcg, da, batch, ar_thunk, &arctx);
                if (drc) return fail(SFMBA_ERR_HIP, "distributed CG: collective failed (rc " + std::to_string(drc) + ")");
                dcg_launched = batch;
            } else {
            if (x32) p->db.shard_blocks32 = reinterpret_cast<float*>(p->d_red); else p->db.shard_blocks = p->d_red;
            with_precision(p, [&](auto t) { launch_schur_pairs<decltype(t)>(p->stream, p->ds, p->db, 1); });
            p->db.shard_blocks = nullptr; p->db.shard_blocks32 = nullptr;
            if (x32) {
                if ((rc = collective(allreduce ? p->allreduce_f32(ctx, p->d_red, shard_offdiag_len(p->ds), (void*)p->stream) : 0, "all-reduce (fp32)"))) return rc;
                launch_shard_offdiag_f32(p->stream, p->ds, F32, reinterpret_cast<const float*>(p->d_red));
            } else {
                if ((rc = reduce(p->d_red, shard_offdiag_len(p->ds)))) return rc;
                launch_shard_offdiag(p->stream, p->ds, p->solver.Sfull, p->d_red, /*unpack=*/true);
                if (F32) launch_narrow_matrix(p->stream, p->solver.Sfull, F32, (long long)p->ds.d * p->ds.ld);
            }
            const int it0 = dense_pcg_solve(p->stream, &p->solver, p->db.S, p->db.rhs, cg_tol, plan.max_iters, p->d_info, nullptr,
                                            { .finish = false, .hist_key = p->shard_host_iter, .pretransformed = true, .anchor = plan.anchor(first_linear_solve), .no_wait = true,
                                              .coarse = coarse_cg });
            first_linear_solve = false;
            if (it0 < 0) return pcg_refused(it0);
            }
            DeviceBuffers dbu = p->db;
            if (f32) dbu.pu32 = p->d_pu32;
            dbu.pcg_vec = p->solver.vec; dbu.pcg_linv = p->solver.binv; dbu.pcg_flags = p->solver.flags;
            dbu.cg_gate = p->solver.flags; dbu.cg_force = 0;
            volatile int* mb = p->h_lm_mail;
            for (;;) {
                with_precision(p, [&](auto t) { launch_back_substitution<decltype(t)>(p->stream, p->ds, dsp, dbu, nullptr); });
                if (!dist_cg) probe_note_solver(p, true, 0);
                else probe_note(p, implicit_cg ? SFMBA_FAMILY_IMPLICIT : row_cg ? SFMBA_FAMILY_DIST_ROWS : SFMBA_FAMILY_DIST_BLOCKS, implicit_cg ? 0 : x32 ? 1 : 0, coarse_cg ? 8 : 0, 0);
                launch_shard_pack(p->stream, p->db, p->d_scal, 2, p->shard_rank);
                if ((rc = reduce(sfmba_shard_scalars_buf(p), SFMBA_SHARD_SCALARS))) return rc;
                dbu.shard_scal = p->d_scal;        // k_lm_control reads the sums from the all-reduced block
                launch_control(p->stream, p->ds, dbu);
                if ((rc = launches_ok())) return rc;
                ++controls;
                // the next linearisation's first kernel before the host waits for the verdict, as in the one-GPU loop (run_solve): it
                // looks at the LM state itself and returns at once if the solve ended or the iteration wants more CG first
                if (speculate && p->shard_host_iter + 2 <= o.max_iters) {
                    with_precision(p, [&](auto t) { launch_point_build<decltype(t)>(p->stream, dsp, p->db, 4); });
                    build_enqueued = true;
                }
                if ((rc = await_control(p, controls, "sharded LM iteration did not complete: ", "no control post"))) return rc;
                if (mb[1] != -2) break;
                if (o.verbose) std::fprintf(stderr, "[sfmba shard %d/%d] CG batch too short after %d launches\n", p->shard_rank, p->shard_world, dist_cg ? dcg_launched : -1);
                // the CG batch was too short (identically on every rank: same matrix, same arithmetic): more iterations, then the trio again
                // (the early linearisation kernel behind that control kernel has returned without doing anything)
                build_enqueued = false;
                if (dist_cg) {
                    const int more = std::min(8, dcg_max - dcg_launched);
                    if (more <= 0) dbu.cg_force = 1;
                    else {
                        const int drc = dcg_iterate(p->stream, &p->dcg, da, more, ar_thunk, &arctx);
                        if (drc) return fail(SFMBA_ERR_HIP, "distributed CG: collective failed (rc " + std::to_string(drc) + ")");
                        dcg_launched += more;
                    }
                } else if (dense_pcg_more(p->stream, &p->solver, 8, nullptr) == 0) dbu.cg_force = 1;
            }
            dense_pcg_note(&p->solver, p->shard_host_iter, mb[4]);
            if (p->probe_on) p->probe.cg_iters = mb[4];
            p->shard_sum.linear_iters += mb[4];
            if (o.verbose) std::fprintf(stderr, "[sfmba shard %d/%d] LM iteration %d: %d CG iterations (%d launched), termination %d\n", p->shard_rank, p->shard_world, mb[3], mb[4], dist_cg ? dcg_launched : 0, mb[1]);
            p->shard_host_iter = mb[3];
            if (shard_terminated(p, mb[1], mb[2])) { limit_exit = mb[1] == -1; break; }
            // one rank (the matrix-free solve of an unsharded handle): the wall-clock limit of the reference (BA.cpp:176) applies; between
            // ranks it cannot (they would disagree on it)
            if (p->shard_world == 1 && o.max_seconds > 0.0 && now_seconds() - t_shard0 >= o.max_seconds) {
                set_termination(p->shard_sum, SFMBA_NO_CONVERGENCE, MSG_MAX_TIME);
                limit_exit = true;
                break;
            }
        }
        if (limit_exit && p->no_pairs && !p->sharded) {
            // The matrix-free solve of an unsharded handle (solve_matrix_free) returns a trace; the sharded entry point returns none and
            // keeps its count, whatever the number of ranks: a run that a LIMIT ends behind an accepted step reports the gradient AT the accepted
            // point in that step's row, and counts the evaluation, as run_solve does (lm_solve.hip) -- the point is linearised once more, up to the
            // kernel that does the post-linearisation bookkeeping (k_pcg_glue).  The limit keeps its precedence over the gradient tolerance.
            if ((rc = download_state(p))) return rc;
            if (p->h_state->termination == -1 && p->h_state->x_is_new) {
                if (!build_enqueued) with_precision(p, [&](auto t) { launch_point_build<decltype(t)>(p->stream, dsp, p->db, 0); });
                with_precision(p, [&](auto t) { launch_cam_diag<decltype(t)>(p->stream, dsc, p->db); });
                launch_cd_fold(p->stream, p->ds, p->db);
                launch_shard_diag(p->stream, p->ds, p->db, p->d_red, /*unpack=*/false, p->shard_rank, p->shard_world);
                if ((rc = reduce(p->d_red, shard_diag_len(p->ds)))) return rc;
                launch_shard_diag(p->stream, p->ds, p->db, p->d_red, /*unpack=*/true, p->shard_rank, p->shard_world);
                { DeviceBuffers dbf = p->db; dbf.cd_part = nullptr; launch_finalize(p->stream, p->ds, dbf, 1); }
                launch_pcg_glue(p->stream, p->ds, p->db);
                if ((rc = launches_ok())) return rc;
                if ((rc = download_state(p))) return rc;
                if (p->h_state->termination == SFMBA_FAILURE) set_termination(p->shard_sum, p->h_state->termination, p->h_state->message);
            }
        }
        if (row_cg) {
            // every rank has moved its own points only: the final points of all ranks, so that the handle holds the whole solution
            if ((rc = download_state(p))) return rc;
            if ((rc = gather(p->db.pts[p->h_state->cur], (size_t)p->own_pt_stride * 3 * sizeof(double)))) return rc;
        }
        return sfmba_shard_end(p, summary);
    }
    for (;;) {
        if ((rc = sfmba_shard_partial_build(p))) return rc;
        if ((rc = reduce(sfmba_shard_reduce_buf(p), sfmba_shard_reduce_len(p)))) return rc;
        if ((rc = sfmba_shard_solve_update(p))) return rc;
        if ((rc = reduce(sfmba_shard_scalars_buf(p), SFMBA_SHARD_SCALARS))) return rc;
        // accept / reject on the device; the host meets the GPU at the control kernel's mailbox post (no copy, no stream sync)
        launch_shard_unpack(p->stream, p->db, p->d_scal, 2, p->shard_world);
        launch_control(p->stream, p->ds, p->db);
        if ((rc = launches_ok())) return rc;
        ++controls;
        volatile int* mb = p->h_lm_mail;
        if ((rc = await_control(p, controls, "sharded LM iteration did not complete: ", "no control post"))) return rc;
        p->shard_host_iter = mb[3];
        if (shard_terminated(p, mb[1], mb[2])) break;
    }
    return sfmba_shard_end(p, summary);
}

int sfmba_problem_solve_sharded(sfmba_problem* p, const sfmba_options* opt, sfmba_allreduce_fn allreduce, void* ctx, sfmba_summary* summary) {
    if (const int hrc = check_handle(p, /*may_be_empty=*/false)) return hrc;
    if (!p->sharded) return fail(SFMBA_ERR_INVALID_ARG, "not a sharded problem (sfmba_problem_create_sharded)");
    return solve_sharded_impl(p, opt, allreduce, ctx, summary);
}

int sfmba_problem_set_allgather(sfmba_problem* p, sfmba_allgather_fn allgather) {
    if (!p) return fail(SFMBA_ERR_INVALID_ARG, "NULL problem");
    p->allgather = allgather;
    return SFMBA_OK;
}

int sfmba_problem_set_reduce_scatter(sfmba_problem* p, sfmba_reduce_scatter_fn reduce_scatter) {
    if (!p) return fail(SFMBA_ERR_INVALID_ARG, "NULL problem");
    p->reduce_scatter = reduce_scatter;
    return SFMBA_OK;
}

int sfmba_shard_last_exchange(const sfmba_problem* p, int64_t out[4]) {
    if (!p || !out) return fail(SFMBA_ERR_INVALID_ARG, "NULL argument");
    for (int k = 0; k < 4; ++k) out[k] = p->shard_exchange[k];
    return SFMBA_OK;
}

int sfmba_problem_set_allreduce_f32(sfmba_problem* p, sfmba_allreduce_f32_fn allreduce_f32) {
    if (const int hrc = check_handle(p)) return hrc;
    p->allreduce_f32 = allreduce_f32;
    return SFMBA_OK;
}
}  // extern "C"

// The matrix-free solve of an UNSHARDED problem without a pair list (include/sfmba.h, SFMBA_CREATE_NO_PAIR_LIST): the CG loop of the sharded
// path on one rank with the reduced matrix applied implicitly (implicit_schur.hip) -- two passes over the observations per CG iteration,
// nothing of size (pairs) or (cameras^2) is ever formed.  The trace rows are the ones k_lm_control wrote.
int sfmba::solve_matrix_free(sfmba_problem* p, const sfmba_options& o, sfmba_summary* summary, sfmba_iteration* trace, int trace_cap, int* trace_len) {
    if (trace_len) *trace_len = 0;
    if (const int hrc = check_handle(p)) return hrc;
    sfmba_summary sum;
    int rc = solve_sharded_impl(p, &o, nullptr, nullptr, &sum);
    if (rc) return rc;
    const int rows = std::min(sum.iterations + 1, p->db.trace_cap);
    if (rows > 0 && (trace || trace_len)) {
        std::vector<TraceRow> tr((size_t)rows);
        if ((rc = read_trace_rows(p, tr.data(), rows))) return rc;
        copy_trace_out(tr.data(), rows, trace, trace_cap, trace_len);
    }
    if (summary) *summary = sum;
    return SFMBA_OK;
}
