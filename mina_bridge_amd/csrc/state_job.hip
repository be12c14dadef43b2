// state_job.hip -- how ONE Proof-of-State job is queued over the lanes and streams of a context (ctx.h StateJobPlan, StreamPlan): the stream of each leg, the events
// that tie the legs together, where the verdict kernel goes.  Host code only, no kernel and no launch: the device is reached through functions declared in ctx.h and
// below, so the file also builds as C++ against the stand-in runtime of tests/fuzz/hip_stub (trace_state_job.cpp; its call order is held by tests/test_state_job_trace.py).
#include "ctx.h"

namespace mb {   // api_kimchi.hip
struct KimchiIn { const uint32_t *pub, *prev_chals, *prev_comms, *w_comm, *z_comm, *t_comm, *evals, *ft_eval1, *pubcomm; };
struct KimchiOut { uint32_t *sponge_state, *sponge_pos, *cip, *evalpoints, *polyscale, *evalscale, *comms, *ft_eval0; };
}
int mb_kimchi_to_batch_dev(mina_ctx *c, size_t batch, uint32_t n_prev, uint32_t npub, const mb::KimchiIn &in, const mb::KimchiOut &out, uint32_t *d_bad, mb::IpaExpand *expand,
                           const void *pf_digest, uint32_t pf_stride);

// Fork / join of a job's legs.  A job may run its three independent legs (protocol states / wrap opening / accumulator) on three lanes -- the current one plus
// helper lanes -- joined by events before the verdict kernel: for small, latency-bound batches the serial chain of dependent Poseidon permutations of one leg
// hides behind the other legs (mina_state_job_batch), large ones fill the chip with fewer jobs in flight (dev_fork_lanes, the boundary's setup_legs).
// `then` waits for what is queued on `first` so far, through the leg event of `owner` (a fork: the forking lane's; a join: the leg's), recorded right above the wait
static int leg_order(Lane &owner, hipStream_t first, hipStream_t then) {
    if (!owner.ev_leg) HIPC(hipEventCreateWithFlags(&owner.ev_leg, hipEventDisableTiming));
    HIPC(hipEventRecord(owner.ev_leg, first));
    HIPC(hipStreamWaitEvent(then, owner.ev_leg, 0));
    return MINA_OK;
}
// Early start of a job's protocol-state leg: the boundary (api_verify.hip) streams the records of a chunk to the GPU while the rest of the
// chunk is still being parsed, and queues the hashes of states [lo, lo + cnt) -- of a job of `ns_total` states whose state leg will run on
// lane LS -- behind `after` (the upload of those records).  The caller keeps count and hands it to mb_state_jobs_on_lane as StateJobPlan::hashed_early.
int mb_state_hashes_early(mina_ctx *c, Lane *LS, size_t ns_total, size_t lo, size_t cnt, const uint32_t *d_records, const uint32_t *d_nfields, hipEvent_t after, HashLaunch hash) {
    if (!LS || lo + cnt > ns_total) return fail(MINA_ERR_ARG, "bad early state range");
    if (!c->have_state_salts) return fail(MINA_ERR_STATE, "call mina_state_jobs_prepare first");
    if (!LS->stream) HIPC(hipStreamCreateWithFlags(&LS->stream, hipStreamNonBlocking));
    int rc;
    if ((rc = LS->st_hashes.ensure(ns_total * 32))) return rc;
    if (after) HIPC(hipStreamWaitEvent(LS->stream, after, 0));
    Lane *const L0 = c->L;
    c->L = LS;
    rc = pstate_hash_dev(c, cnt, ns_total, hash, d_records + lo * MINA_PSTATE_SLOTS * 8, d_nfields + lo, LS->st_hashes.as<uint32_t>() + lo * 8, nullptr);
    c->L = L0;
    return rc;
}

// ---- the legs of a job.  Each is told its lane and makes it the current one (c->L: where every mb_*_dev helper queues); mb_state_jobs_on_lane restores the
// caller's.  Every pointer of `j` is a device pointer; nothing here waits for the GPU.  `v` collects the words the verdict kernel reads.

// protocol-state leg: the hashes of the job's states (those not queued early), then the chain check -> S.st_ok
static int state_leg(mina_ctx *c, const mina_state_jobs *j, Lane &S, const StateJobPlan &plan) {
    c->L = &S;
    const size_t B = j->batch;
    int rc;
    if (j->with_states) {
        const size_t ns = B * MINA_STATES_PER_PROOF;
        if ((rc = S.st_hashes.ensure(ns * 32))) return rc;
        const size_t early = std::min(plan.hashed_early, ns);          // already queued on this lane by mb_state_hashes_early
        const uint32_t *rec = (const uint32_t *)j->state_records, *nf = (const uint32_t *)j->state_nfields;
        // mina_ctx_set_state_dedup: the whole leg at once, each distinct record hashed once (a piece queued early could not know its duplicates in later pieces)
        if (c->state_dedup && early == 0) {
            if ((rc = pstate_hash_dedup_dev(c, ns, ns, plan.hash, rec, nf, S.st_hashes.as<uint32_t>(), nullptr, true))) return rc;
        } else if (early < ns && (rc = pstate_hash_dev(c, ns - early, ns, plan.hash, rec + early * MINA_PSTATE_SLOTS * 8, nf + early, S.st_hashes.as<uint32_t>() + early * 8, nullptr))) return rc;
        mb_launch_pstate_chain_check(S.stream, (uint32_t)B, S.st_hashes.as<uint32_t>(), (const uint32_t *)j->expected_hashes, rec, (const uint8_t *)j->precheck, S.st_ok.as<uint32_t>());
    } else {
        // no state leg: chain_ok = all ones
        if (j->precheck) return fail(MINA_ERR_ARG, "precheck needs the protocol-state section");
        mb_launch_fill_u32(S.stream, (uint32_t)B, 1u, S.st_ok.as<uint32_t>());
    }
    HIPC(hipGetLastError());
    return MINA_OK;
}

// accumulator leg: the folded check of the step accumulators -> v.acc_v
static int accumulator_leg(mina_ctx *c, const mina_state_jobs *j, Lane &A, const FoldExport *fx, StateJobCarry &v) {
    c->L = &A;
    if (!j->with_accumulator) return MINA_OK;
    const size_t B = j->batch;
    int rc;
    if ((rc = A.st_flags.ensure(16 * 4))) return rc;
    v.acc_v = A.st_flags.as<uint32_t>() + 8;
    return mb_accumulator_check_dev(c, CURVE_VESTA, j->acc_k, B, (const uint32_t *)j->acc_prechallenges, (const uint32_t *)j->acc_sg, B > 1 ? (const uint32_t *)j->acc_rho : nullptr, v.acc_v, fx);
}

// wrap-proof leg: Pickles statement -> public-input commitment -> kimchi to_batch -> combined opening check; -> v.stmt_ok, v.kimchi_bad, v.ipa_v
// check: the stream of the opening check (JobRoute::check).  Where it is not the lane's own -- the role plan (ctx.h StreamPlan): W2 -- the leg has two stages, cut in
// front of the opening check: everything before runs on the lane's stream (W1), the opening check on `check` behind ONE event recorded on W1.
// mb_ipa_batch_check_dev queues on the current lane's stream: for the length of that call, and no longer, the lane's handle names `check` (OnStream).
struct OnStream { hipStream_t &handle; const hipStream_t own; OnStream(Lane &l, hipStream_t s) : handle(l.stream), own(l.stream) { handle = s; } ~OnStream() { handle = own; } };
// d_net (StateJobPlan::d_net): a mixed job -- the two stages that read index data run in their `_net` forms, through the context's pointers.
static int wrap_leg(mina_ctx *c, const mina_state_jobs *j, Lane &L, const FoldExport *fx, StateJobCarry &v, hipStream_t check, const uint8_t *d_net, bool count) {
    c->L = &L;
    if (d_net && j->kimchi && (!c->pickles_statements_net || !c->kimchi_to_batch_net)) return fail(MINA_ERR_STATE, "this context cannot queue a mixed job");
    const size_t B = j->batch;
    int rc;
    auto to_check = [&]() -> int { return check == L.stream ? MINA_OK : leg_order(L, L.stream, check); };
    auto opening_check = [&](const mb::IpaShape &sh, const mb::IpaDevIn &in) -> int {
        if ((rc = to_check())) return rc;
        OnStream on(L, check);
        return mb_ipa_batch_check_dev(c, CURVE_PALLAS, sh, in, v.ipa_v, fx);
    };
    if ((rc = L.st_flags.ensure(16 * 4))) return rc;
    const uint32_t *pub = (const uint32_t *)j->public_inputs, *comm_override = nullptr;
    if (j->kimchi && j->kimchi->statements) {      // the Pickles statement -> the wrap circuit's public inputs, on this lane ahead of everything that reads them
        if ((rc = L.pk_pub.ensure(B * 40 * 32)) || (rc = L.pk_ok.ensure(B * 4))) return rc;
        if ((rc = d_net ? c->pickles_statements_net(c, B, j->kimchi->statements, L.pk_pub.as<uint32_t>(), L.pk_ok.as<uint32_t>(), d_net)
                        : mb_pickles_statements_dev(c, B, j->kimchi->statements, L.pk_pub.as<uint32_t>(), L.pk_ok.as<uint32_t>()))) return rc;
        pub = L.pk_pub.as<uint32_t>(); v.stmt_ok = L.pk_ok.as<uint32_t>();
    }
    if (j->npub || j->kimchi) {
        if ((rc = L.st_pubcomm.ensure(B * 64))) return rc;
        if ((rc = mb_pubcomm_dev(c, B, j->log2_domain, j->npub, pub, L.st_pubcomm.as<uint32_t>()))) return rc;
        comm_override = L.st_pubcomm.as<uint32_t>();
    }
    if (!j->with_ipa) return to_check();
    mb::IpaShape sh; sh.batch = (uint32_t)B; sh.k = j->k; sh.npts = j->n_evalpoints; sh.ncomms = j->n_comms; sh.per = 2 * j->k + j->n_comms + 4;
    auto W = [](const void *p) { return (const uint32_t *)p; };
    v.ipa_v = L.st_flags.as<uint32_t>() + 4;
    if (!j->kimchi) {
        sh.override_slot = j->npub ? j->pub_comm_slot : 0xffffffffu;
        mb::IpaDevIn in{W(j->sponge_state), W(j->sponge_pos), W(j->cip), W(j->lr), W(j->delta), W(j->sg), W(j->z1), W(j->z2), W(j->evalpoints), W(j->evalscale),
                        W(j->polyscale), W(j->comms), comm_override, W(j->rand_base), W(j->sg_rand_base)};
        return opening_check(sh, in);
    }
    // kimchi oracles + to_batch produce the BatchEvaluationProof rows in lane buffers (the public-input commitment is already in the list)
    const mina_kimchi_proofs &kp = *j->kimchi;
    if ((rc = L.kc_state.ensure(B * 96)) || (rc = L.kc_pos.ensure(B * 8)) || (rc = L.kc_cip.ensure(B * 32)) || (rc = L.kc_pts.ensure(B * 64)) ||
        (rc = L.kc_v.ensure(B * 32)) || (rc = L.kc_u.ensure(B * 32)) || (rc = L.kc_comms.ensure(B * (size_t)j->n_comms * 64))) return rc;
    v.kimchi_bad = L.st_flags.as<uint32_t>() + 12;
    HIPC(hipMemsetAsync(v.kimchi_bad, 0, 4, L.stream));
    const uint32_t *prev_chals = W(kp.prev_chals);
    // no recursion challenges given beside a statement: they ARE the statement's messages_for_next_wrap_proof.old_bulletproof_challenges
    // (2 x 15; the one source a verifier has), and their digest was taken on the way by the statement stage
    const bool from_statement = !kp.prev_chals && !kp.prev_prechallenges && kp.statements && kp.n_prev == 2 && j->k == 15;
    const void *pre = from_statement ? kp.statements->wrap_old_challenges : kp.prev_prechallenges;
    const void *pf_digest = nullptr; uint32_t pf_stride = 0;
    if (from_statement && mb_tune().kimchi_shared_digest) mb_pickles_kimchi_digest(c, kp.statements, &pf_digest, &pf_stride);
    if (pre && kp.n_prev) {                             // 128-bit prechallenges -> scalar-field challenges, on this lane ahead of the sponges
        const size_t cnt = B * kp.n_prev * j->k;
        if ((rc = L.kc_pch.ensure(cnt * 32))) return rc;
        mb_launch_challenge_to_field_fq(L.stream, (uint32_t)cnt, c->fk[FIELD_FQ], W(pre), L.kc_pch.as<uint32_t>());
        prev_chals = L.kc_pch.as<uint32_t>();
    }
    mb::KimchiIn in{pub, prev_chals, W(kp.prev_comms), W(kp.w_comm), W(kp.z_comm), W(kp.t_comm), W(kp.evals), W(kp.ft_eval1), comm_override};
    mb::KimchiOut out{L.kc_state.as<uint32_t>(), L.kc_pos.as<uint32_t>(), L.kc_cip.as<uint32_t>(), L.kc_pts.as<uint32_t>(), L.kc_v.as<uint32_t>(), L.kc_u.as<uint32_t>(),
                      L.kc_comms.as<uint32_t>(), nullptr};
    mb::IpaDevIn iin{out.sponge_state, out.sponge_pos, out.cip, W(j->lr), W(j->delta), W(j->sg), W(j->z1), W(j->z2), out.evalpoints, out.evalscale, out.polyscale,
                     out.comms, nullptr, W(j->rand_base), W(j->sg_rand_base)};
    if (d_net) {
        // The index commitments differ between the proofs of a mixed job: the ft row is computed per proof (no expanded slot) and h is the one batch-shared point.
        if (count && (rc = mb_ctx_mixed_totals(c))) return rc;
        if ((rc = c->kimchi_to_batch_net(c, B, kp.n_prev, kp.npub, in, out, v.kimchi_bad, d_net, pf_digest, pf_stride, count ? c->mixed_totals.p : nullptr))) return rc;
        if (mb_tune().ipa_shared_points) { sh.shared_h = 1; sh.nshared = 1; }
        return opening_check(sh, iin);
    }
    mb::IpaExpand ex;
    if ((rc = mb_kimchi_to_batch_dev(c, B, kp.n_prev, kp.npub, in, out, v.kimchi_bad, &ex, pf_digest, pf_stride))) return rc;
    sh.expand_slot = kp.n_prev + 1; sh.per += mb::IPA_EXPAND - 1;          // the ft commitment enters the MSM as its 8 terms
    if (mb_tune().ipa_shared_points && kp.n_prev + 45 <= 64) {   // h, the 27 index columns and the index point of the ft combination are the same
        uint64_t m = 0;                                                       // points for every proof: their scalars are summed first (29 of 88 entries per proof)
        for (uint32_t i = kp.n_prev + 3; i < kp.n_prev + 9; ++i) m |= (uint64_t)1 << i;        // 6 selectors
        for (uint32_t i = kp.n_prev + 24; i < kp.n_prev + 45; ++i) m |= (uint64_t)1 << i;      // 15 coefficients + 6 sigma
        sh.shared_lo = (uint32_t)m; sh.shared_hi = (uint32_t)(m >> 32); sh.shared_h = 1; sh.shared_expand0 = 1; sh.nshared = 29;
    }
    iin.expand = ex;
    return opening_check(sh, iin);
}

// ---- the route of ONE job: resolved once from the caller's plan (ctx.h StateJobPlan) and the current lane; one body (mb_state_jobs_on_lane) then queues every shape.
// lane: the current lane on entry.  wrap / acc / states: the lane of each leg -- its workspaces and, through its `stream`, where its work goes; `lane` itself where
// the job does not fork.  `lane` keeps the fork, the joins and the verdict kernel on its own stream, except under the role plan (ctx.h StreamPlan, plan B): there
// NOTHING is queued on it (a wait on its stream would be a barrier in whatever hardware queue that stream shares) and the job flows through the role streams, FIFO
// behind the jobs queued before it -- H: the state hashes, the chain check; W2: the accumulator check; W1: the first stage of the wrap-proof leg, then ONE event
// W1 -> W2 (wrap_leg); W2: the opening check, ONE event H -> W2, the verdict kernel, the lane's `done` event.  The helper lanes lend their workspaces (each job in
// flight has its own); the NEXT job of `lane` reuses them, so it begins with H, W1 and W2 waiting for `done` (long completed, with two lanes or more).
// With two hash carriers (ctx.h StreamPlan::carriers) "H" is the carrier of the job's lane, H or H1 -- a lane keeps its carrier for as long as the plan holds, so
// `done` covers its workspaces as before -- and the opening check of every other lane stays on W1 behind kimchi (check_on_wrap): W2 then joins W1 behind the
// check, by the event that otherwise stands in front of it.
// Invariant (held by tests/test_state_job_trace.py): every wait names an event recorded EARLIER in host submission order -- each record stands above the waits on
// it, `done` was recorded by the lane's previous job (Lane::on_roles guards the first) -- and every stream is fed in submission order: the graph cannot cycle.
struct JobRoute {
    Lane *lane, *wrap, *acc, *states;
    bool roles = false, acc_ahead = false;      // roles: begins with waits for `done` and ends by recording it, instead of fork and join on `lane`; acc_ahead: LegStreams::acc_first
    bool check_on_wrap = false;                 // roles with two hash carriers, every other lane (ctx.h StreamPlan::check_on_w1): the opening check follows kimchi on W1, and W2 joins W1 as it joins H
    hipStream_t home() const { return roles ? acc->stream : lane->stream; }       // gets the joins and the verdict kernel: the lane's own stream, or W2
    hipStream_t check() const { return roles && !check_on_wrap ? acc->stream : wrap->stream; }      // the opening check's: the wrap-proof leg's own stream, or W2
};
// plan.wrap / .acc: helper lanes of the wrap-proof and accumulator legs (null = everything on the current lane, in order); plan.states: a lane of its own for the
// protocol-state leg as well (the boundary gives the chain and the hashes streams with disjoint CU masks, api_verify.hip)
static JobRoute resolve_route(mina_ctx *c, const StateJobPlan &plan) {
    Lane *const L0 = c->L;
    JobRoute r{L0, L0, L0, L0};
    if (!(plan.wrap && plan.acc && plan.wrap != L0 && plan.acc != L0 && plan.wrap != plan.acc)) return r;
    r.wrap = plan.wrap; r.acc = plan.acc;
    if (plan.states && plan.states != L0 && plan.states != r.wrap) r.states = plan.states;      // states == acc: the accumulator leg shares the hashes' stream (behind them, or ahead)
    if (const LegStreams *lent = plan.lent) {      // the ONE place a helper lane is handed a stream: it holds for this job
        r.wrap->stream = lent->wrap; r.acc->stream = lent->acc; r.states->stream = lent->states;
        r.roles = lent->roles; r.acc_ahead = lent->acc_first && r.acc == r.states; r.check_on_wrap = lent->roles && lent->check_on_wrap;
    }
    return r;
}

// One job, queued from the current lane along its route.  plan.phase: MB_JOB_ALL queues the whole job.  The boundary queues a job in two steps, because the
// wrap-proof half of its input is parsed (and uploaded) before the protocol states are: MB_JOB_LEGS = the accumulator and wrap-proof legs (their verdict pointers
// are kept in plan.carry), later MB_JOB_FINISH = the protocol-state leg (minus the plan.hashed_early states mb_state_hashes_early queued already), the joins and the verdict kernel.
int mb_state_jobs_on_lane(mina_ctx *c, const mina_state_jobs *j, uint32_t *d_verdicts, uint32_t *d_flags, const StateJobPlan &plan) {
    const uint32_t phase = plan.phase;
    if (phase != MB_JOB_ALL && !plan.carry) return fail(MINA_ERR_ARG, "a split job needs a carry");
    const JobRoute r = resolve_route(c, plan);
    Lane &L0 = *r.lane, &LI = *r.wrap, &LA = *r.acc, &LS = *r.states;
    struct Restore { mina_ctx *c; Lane *l0; ~Restore() { c->L = l0; } } restore{c, &L0};      // the legs switch the current lane: back to the caller's on every return
    int rc;
    if (r.roles) {
        if (!L0.ev_done) HIPC(hipEventCreateWithFlags(&L0.ev_done, hipEventDisableTiming));
        // the lane's last job ran under plan A (its verdict kernel on the lane's own stream), or another entry point used the lane: behind that
        if (!L0.on_roles) { HIPC(hipEventRecord(L0.ev_done, L0.stream)); L0.on_roles = true; }
        for (hipStream_t s : {LS.stream, LI.stream, r.home()}) HIPC(hipStreamWaitEvent(s, L0.ev_done, 0));
    } else {
        // a lent lane whose last job ran under plan B: its helper lanes' workspaces are free behind that job's `done` event
        if (plan.lent && L0.on_roles) { HIPC(hipStreamWaitEvent(L0.stream, L0.ev_done, 0)); L0.on_roles = false; }
        auto fork = [&](Lane &to) -> int {
            if (&to != &L0 && !to.stream) HIPC(hipStreamCreateWithFlags(&to.stream, hipStreamNonBlocking));
            return &to == &L0 ? MINA_OK : leg_order(L0, L0.stream, to.stream);
        };
        if ((phase & MB_JOB_LEGS) && ((rc = fork(LI)) || (rc = fork(LA)))) return rc;
        if ((phase & MB_JOB_FINISH) && (rc = fork(LS))) return rc;      // (states == acc: forked a second time, as it is joined a second time below)
    }
    const size_t B = j->batch;
    if (plan.d_net && plan.count_mixed && (phase & MB_JOB_LEGS)) ++c->mixed_jobs;      // mina_ctx_mixed_job_stats (the proofs are counted on the device: wrap_leg)
    StateJobCarry v;                                            // what the legs leave for the verdict kernel; the first leg that fails ends them (rc)
    rc = r.acc_ahead ? accumulator_leg(c, j, LA, plan.fold_export, v) : MINA_OK;
    if (!rc) rc = LS.st_ok.ensure(B * 4);                       // the chain_ok words, in either phase
    if (!rc && (phase & MB_JOB_FINISH)) rc = state_leg(c, j, LS, plan);
    if (!rc && (phase & MB_JOB_LEGS)) {
        // The accumulator leg shares scratch buffers with the opening check (ipa_chals / ipa_sigma / ipa_points of its lane), and the
        // culprit search re-checks slices of a failed batch from the rows the opening check LEFT in those buffers (mb_ipa_recheck_rows): on the
        // wrap leg's own lane the accumulator therefore runs FIRST (run after it, as it did until round 3, it overwrote the rows: every
        // part of a search then failed and a batch of more than 1024 proofs with one bad opening was rejected whole).  Under the role plan it shares
        // the opening check's STREAM: first as well, so that W2 has work while W1 runs the first stage of the wrap-proof leg.
        const bool before = &LA == &LI || r.roles;
        if (before && !r.acc_ahead) rc = accumulator_leg(c, j, LA, plan.fold_export, v);
        if (!rc) rc = wrap_leg(c, j, LI, plan.fold_export, v, r.check(), plan.d_net, plan.count_mixed);
        if (!rc && !before && !r.acc_ahead) rc = accumulator_leg(c, j, LA, plan.fold_export, v);
    }
    if (!rc && phase == MB_JOB_LEGS) { *plan.carry = v; return MINA_OK; }      // the legs stay forked: MB_JOB_FINISH joins them
    if (phase == MB_JOB_FINISH) v = *plan.carry;
    // The joins: the home stream waits for every leg that ended on another stream (the wrap-proof leg: on the opening check's).  states == acc: that lane is joined a
    // second time -- redundant, and what this code has always queued.  A job whose leg FAILED is joined too (its wrap-proof leg may have stopped short of the check
    // stream) and ends as a good one does, less the verdict kernel: what its legs queued reads the caller's inputs on streams mina_ctx_synchronize does not wait for
    // (mina_ctx::fork_own).  The role streams are FIFO and mb_ctx_wait_all waits for them: there the caller needs no more, but a lane pinned next runs under plan A
    // behind `done` alone, which therefore stands behind everything the failed job queued.
    const hipStream_t home = r.home();
    const struct { Lane &leg; hipStream_t from; } ends[3] = {{LI, rc ? LI.stream : r.check()}, {LA, LA.stream}, {LS, LS.stream}};
    for (const auto &e : ends) if (e.from && e.from != home) { const int jrc = leg_order(e.leg, e.from, home); if (jrc && !rc) return jrc; }
    if (!rc) mb_launch_state_job_verdict(home, (uint32_t)B, LS.st_ok.as<uint32_t>(), v.ipa_v, v.acc_v, v.kimchi_bad, v.stmt_ok, d_verdicts, d_flags, plan.d_stmt_out);
    if (!rc) HIPC(hipGetLastError());
    if (r.roles && hipEventRecord(L0.ev_done, home) != hipSuccess && !rc) return fail(MINA_ERR_HIP, "hipEventRecord failed");
    return rc;
}

// The legs of a device-resident job on streams of their own (mina_verify_tuning.dev_fork).  One stream per job needs ~20 jobs in flight to
// fill the chip: the wrap-proof chain is ~15 dependent kernels of 781 waves (16 384 proofs in the 3-lane form) on 1024 SIMDs, and nothing of the SAME job may run
// beside them -- 47.6 GiB of workspaces and 71 ms of call latency for the headline.  The three legs of a job are independent until the verdict kernel (the same
// split the boundary makes per chunk, api_verify.hip setup_legs): pipeline lane i keeps the fork / join and the verdict kernel, its helper lanes
// MB_DEV_HELPER0 + 3 i + {0, 1, 2} run the wrap-proof chain, the accumulator check and the state hashes.  Streams are created once per context under the tuning
// then in force (a stream keeps its CU mask / priority for life).  A pinned lane (mina_ctx_pin_lane: the caller queues its own work on that lane's stream) forks as well: the legs
// start behind an event recorded on the lane and the lane waits for them before its verdict kernel, so everything the caller queued before the call is seen by every leg and
// everything it queues after the call sees every leg's output -- the exchange variant (mina_state_job_fold_dev under sharded.py's `ordered()` scope) keeps its ONE ordering stream.
// That is plan A of ctx.h stream_plan: 4 streams per lane, taken when they fit the context's stream budget (GPU_MAX_HW_QUEUES less the null stream's queue, or
// mina_ctx_set_stream_budget), for a lone job and for a pinned context.  Otherwise plan B: the helper lanes lend their workspaces and the job flows through the
// context's role streams (JobRoute).  The helper lanes own no stream under either plan: their handles alias mina_ctx::fork_own / ::role, lent per job (ctx.h LegStreams).
// Fills in the lanes and the hash launch of `plan` and the streams of `lend`; a job that does not fork keeps both as they came (everything on the current lane, one launch).
static int dev_fork_lanes(mina_ctx *c, size_t leg_states, StateJobPlan &plan, LegStreams &lend) {
    const mina_verify_tuning tu = mb_tune();
    const int li = (int)(c->L - c->lanes);
    if (!(tu.dev_fork & 1u) || c->nlanes > MB_DEV_FORK_MAX || li < 0 || li >= MB_DEV_FORK_MAX) return MINA_OK;
    const int in_flight = c->pinned >= 0 ? 1 : c->nlanes;          // a pinned context runs one job at a time
    Lane *h = &c->lanes[MB_DEV_HELPER0 + 3 * li];
    if (c->stream_budget_env < 0) c->stream_budget_env = env_stream_budget();
    const StreamPlan sp = c->stream_budget > 0 ? stream_plan(in_flight, c->stream_budget) : stream_plan_env(in_flight, c->stream_budget_env);
    c->last_plan = sp;
    const uint32_t mode = c->dev_fork_made ? c->dev_fork_made : tu.dev_fork;
    c->dev_fork_made = mode;
    int prio_lo = 0, prio_hi = 0;
    auto make = [&](hipStream_t &st, bool chain, bool masked, int prio) -> int {
        if (st) return MINA_OK;
        int ncu = 0; (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device);
        if (masked && tu.dev_chain_cus > 0 && tu.dev_chain_cus < (uint32_t)ncu && ncu <= 256) {
            // bit i of a mask = CU i / 8 of XCD i % 8 (tools/probes/cumask_probe.hip): the first dev_chain_cus bits are the same CUs of every XCD
            uint32_t mk[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (uint32_t b2 = 0; b2 < (uint32_t)ncu; ++b2) if ((b2 < tu.dev_chain_cus) == chain) mk[b2 >> 5] |= 1u << (b2 & 31);
            if (hipExtStreamCreateWithCUMask(&st, 8, mk) == hipSuccess) return MINA_OK;
            (void)hipGetLastError(); st = nullptr;
        }
        if (prio_lo != prio_hi && (mode & 4u)) HIPC(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, prio));
        else HIPC(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        return MINA_OK;
    };
    int rc;
    if (sp.roles) {
        // plan B: the role streams are the context's, created once (H at the hashes' priority, the chain streams at the chain's; no CU masks: a role serves every job)
        if (!c->role[sp.streams - 1] || (sp.carriers >= 2 && !c->role[MB_ROLE_H1])) (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);      // numerically lower = higher priority
        for (int i = 0; i < sp.streams; ++i) if ((rc = make(c->role[i], true, false, (i == 0 && sp.streams > 1) ? prio_lo : prio_hi))) return rc;
        if (sp.carriers >= 2 && (rc = make(c->role[MB_ROLE_H1], true, false, prio_lo))) return rc;      // the second carrier: at the hashes' priority, as H
        plan.wrap = &h[0]; plan.acc = &h[1]; plan.states = &h[2];
        lend.wrap = c->role[sp.w1(li)]; lend.acc = c->role[sp.w2(li)]; lend.states = c->role[sp.h(li)]; lend.roles = true; lend.check_on_wrap = sp.check_on_w1(li);
    } else {
        hipStream_t *own = &c->fork_own[3 * li];
        if (!own[0] || !own[1] || !own[2]) {
            (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
            if ((rc = make(own[0], true, (mode & 2u) != 0, prio_hi)) || (rc = make(own[1], true, false, (prio_lo + prio_hi) / 2)) || (rc = make(own[2], false, (mode & 2u) != 0, prio_lo))) return rc;
        }
        const int a = tu.dev_acc_lane ? 2 : 1;                                                   // dev_acc_lane: the accumulator leg on the hashes' stream (1: behind them, 2: ahead)
        plan.wrap = &h[0]; plan.acc = &h[a]; plan.states = &h[2];
        lend.wrap = own[0]; lend.acc = own[a]; lend.states = own[2]; lend.acc_first = tu.dev_acc_lane == 2;
    }
    // The hashes of a forked job go out in pieces, so that the jobs in flight together ask for ~6 state-hash waves per SIMD (five fit beside nothing else, 96 VGPRs):
    // measured with the wave priorities on (lanes x piece grid at 4096 / 8192 / 16 384 proofs per call, profiles/r06_dev_fork.md) the best piece is ~6144 / lanes waves
    // whatever the call size -- 2 lanes 3072, 3: 2048, 4: 1536, 6: 1024 -- and a lone call is best left whole.  The single-lane form (ctx.h hash_one_lane) wants twice
    // as many of its waves of 64 states (profiles/r07_one_lane_hash.md, 4 lanes: 768 / 1536 / 3072 waves 253 / 262 / 282 k proofs/s; pieces of the 3-lane form's
    // states, 21 per wave, left a lone wave on half the SIMDs: -13 % on the step).
    // Under the role plan H holds nothing but hashes, one launch behind the other: a piece only leaves wave slots idle until the next one starts, and the leg is
    // best left whole (4 lanes at budget 3, one run each: pieces of 3072 waves 265 k proofs/s, the whole leg of 4352 waves 283 k; profiles/r08_role_streams.md).
    // Under plan A one size above 3072 was tried as well: the whole leg, 315 k against 318 - 321 k -- the default stays.
    // Two carriers hold the pieces of two jobs resident together: equal pieces again (ctx.h role_piece_waves).
    uint32_t piece = tu.dev_piece_waves;
    if (piece == 0 && in_flight >= 2 && !sp.roles) piece = (hash_one_lane(c, leg_states) ? 12288u : 6144u) / (uint32_t)in_flight;
    if (piece == 0 && sp.carriers >= 2) { const bool one = hash_one_lane(c, leg_states); piece = role_piece_waves((leg_states + (one ? 63 : 20)) / (one ? 64 : 21), in_flight, one); }
    if (piece == 0xffffffffu) piece = 0;
    plan.hash.piece_waves = piece;
    // A lone forked job: its hashes would hold every wave slot their 96 VGPRs allow (5 per SIMD) and the chain's waves would wait for one to retire (~13 ms): the
    // hash workgroups reserve 41 KiB of LDS each -- three per CU = 3 waves per SIMD, 224 VGPRs left: room for a wave of every chain kernel but the two PolishToken
    // interpreters (244 / 194 VGPRs + 64 KiB of LDS: they wait for a CU to drain either way).  Lone calls
    // 16 384: 63.6 -> 61.5 ms, 8192: 38.7 -> 36.2 ms; with several jobs in flight the pieces do that job and the reservation costs 1 - 3 % (profiles/r06_dev_fork.md).
    uint32_t lds_kb = tu.dev_hash_lds_kb;
    if (lds_kb == 0 && in_flight == 1) lds_kb = 41;
    if (lds_kb == 0xffffffffu || lds_kb > 160) lds_kb = 0;
    plan.hash.lds_bytes = lds_kb * 1024u;
    return MINA_OK;
}

static int dev_job(mina_ctx *c, const mina_state_jobs *jobs, void *d_verdicts, void *d_flags, StateJobPlan plan) {
    if (!c->have_state_salts && jobs->with_states) return fail(MINA_ERR_STATE, "call mina_state_jobs_prepare first");
    HIPC(hipSetDevice(c->device));
    c->next_lane();
    LegStreams lend;
    if (int rc = dev_fork_lanes(c, jobs->with_states ? jobs->batch * MINA_STATES_PER_PROOF : 0, plan, lend)) return rc;
    if (lend.wrap) plan.lent = &lend;
    return mb_state_jobs_on_lane(c, jobs, (uint32_t *)d_verdicts, (uint32_t *)d_flags, plan);
}

extern "C" int mina_state_job_batch_dev(mina_ctx *c, const mina_state_jobs *jobs, void *d_verdicts, void *d_flags) {
    if (int rc = mb_check_jobs(c, jobs)) return rc;
    if (!d_verdicts) return fail(MINA_ERR_ARG, "null argument");
    return dev_job(c, jobs, d_verdicts, d_flags, StateJobPlan{});
}
// the same job with proofs of both index sets of the context (include/mina_verify.h "MIXED jobs"): one plan field more, the same route
extern "C" int mina_state_job_batch_net_dev(mina_ctx *c, const mina_state_jobs *jobs, const void *d_net, void *d_verdicts, void *d_flags) {
    if (int rc = mb_check_jobs(c, jobs)) return rc;
    if (!d_verdicts || !d_net) return fail(MINA_ERR_ARG, "null argument");
    if (!c->mixed_sets_check) return fail(MINA_ERR_STATE, "this context cannot queue a mixed job");
    if (int rc = c->mixed_sets_check(c)) return rc;
    StateJobPlan plan; plan.d_net = (const uint8_t *)d_net;
    return dev_job(c, jobs, d_verdicts, d_flags, plan);
}

// SURVEY.md 8e.2 for the WHOLE job (the `north_star` variant: "a single reduce of partial sums over xGMI"): this shard's proofs go through every stage of the
// job -- state hashes, statements, kimchi, the opening transcripts, both folds -- but the two fixed-base MSMs and their comparisons are left to the caller,
// who exchanges the shards' folded scalar vectors (all-to-all), commits over its slice of the bases and reduces the partial points (mina_bridge_amd/sharded.py
// ShardedStateJob).  Written here, all in HBM: d_ipa_scalars 2^k x 32 B (Pallas, the wrap openings' sum_b sigma_b s_b), d_ipa_point 17 words (the shard's
// variable-base partial sum of the opening check, to be ADDED to the fixed-base part: the batch passes iff the total is the point at infinity),
// d_acc_scalars 2^acc_k x 32 B (Vesta, sum_b rho_b s_b of the step accumulators), d_acc_point 17 words (sum_b rho_b sg_b: must EQUAL the fixed-base part).
// d_verdicts[b] = every per-proof check of proof b (chain, linkage, statement, well-formed inputs) -- the folded checks are the caller's to AND in.
// Needs at least 2 proofs and both folded legs (with_ipa, with_accumulator).  The folding randomisers of the job are the shard's own (independent of the
// other shards'), and the opening fold's powers start at 1 (rho_b = rand_base^(b+1): IpaShape::pow_first) -- the shards' partials are ADDED, so no proof of any
// shard may carry a fixed coefficient (round 4 shipped ^b: first proofs of two shards with discrepancies +tH / -tH cancelled).
extern "C" int mina_state_job_fold_dev(mina_ctx *c, const mina_state_jobs *jobs, void *d_verdicts, void *d_flags, void *d_ipa_scalars, void *d_ipa_point,
                                       void *d_acc_scalars, void *d_acc_point) {
    if (int rc = mb_check_jobs(c, jobs)) return rc;
    if (!d_verdicts || !d_ipa_scalars || !d_ipa_point || !d_acc_scalars || !d_acc_point) return fail(MINA_ERR_ARG, "null argument");
    if (jobs->batch < 2 || !jobs->with_ipa || !jobs->with_accumulator || !jobs->acc_rho) return fail(MINA_ERR_ARG, "the exchange variant needs >= 2 proofs and both folded legs");
    const FoldExport fe{(uint32_t *)d_ipa_scalars, (uint32_t *)d_ipa_point, (uint32_t *)d_acc_scalars, (uint32_t *)d_acc_point};
    StateJobPlan plan; plan.fold_export = &fe;
    return dev_job(c, jobs, d_verdicts, d_flags, plan);
}
