// trace_state_job.cpp -- the call trace of ONE Proof-of-State job's host orchestration (mina_bridge_amd/csrc/state_job.hip: which stream each leg runs on, which
// events tie the legs together, where the verdict kernel goes), one layer below tsan_boundary.cpp's `trace` mode, which stubs that layer out.
//
// What is built (`make -C tests/fuzz trace_job`): the product's state_job.hip and host_core.hip, compiled as C++ against the stand-in runtime of hip_stub/ with its
// call log on (-DMB_STUB_TRACE).  What is stubbed, below: the device layer beneath them -- the argument checks, the state hashes, the four launch functions
// (api_state.hip), the opening / accumulator checks, kimchi, the Pickles statement stage, the public-input commitment -- and the context.  Each stub prints one
// line: its name, the batch, the index of the current lane in c->lanes and the trace name of that lane's stream -- a launch function, which is told its stream and
// does not look at the current lane: its name, the batch and that stream.
// A stub leg fails on a marker in the job: the first word of state_nfields (state leg), of lr (wrap-proof leg) or of acc_prechallenges (accumulator leg) = BAD.
//
// What runs: a fixed script from one thread; `# ` heads every scenario.  tests/test_state_job_trace.py compares the output with
// tests/golden/state_job_call_trace.txt and checks that every wait names an event recorded earlier.
//
// The lane triples (wrap, acc, states) the boundary's setup_legs (api_verify.hip ShapePass) can produce for a chunk on pipeline lane s, helper lanes h = 32 + 3 s:
//   (null, null, null)         more chunks in flight than mina_verify_tuning.split_max: the whole job on the chunk's lane
//   (h, h + 1, h + 2)          three helper lanes (their streams CU-masked, or plain where the runtime has no masks)
//   (h, h + 1, null)           chain_cus = 0 or >= the CUs of the device: no masks, the protocol-state leg stays on the chunk's lane
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../mina_bridge_amd/csrc/ctx.h"

// ------------------------------------------------------------------------------------------------ the stub device layer
static constexpr uint32_t BAD = 0x21444142u;      // "BAD!"
static mina_ctx *g_ctx = nullptr;                 // the context of the running scenario (the launch functions get none)
static bool marked(const void *p) { return p && *(const uint32_t *)p == BAD; }
static void say(const char *name, size_t batch, const char *fmt = nullptr, ...) {
    const mina_ctx *c = g_ctx;
    printf("%s batch %zu", name, batch);
    if (strncmp(name, "mb_launch_", 10)) printf(" lane %d s%d", (int)(c->L - c->lanes), mb_stub_id(c->L->stream));
    if (fmt) { va_list ap; va_start(ap, fmt); vprintf(fmt, ap); va_end(ap); }
    printf("\n");
}
int mb_check_jobs(mina_ctx *, const mina_state_jobs *j) { say("mb_check_jobs", j->batch); return MINA_OK; }
int mb_pickles_check(mina_ctx *, const mina_pickles_statements *) { return MINA_OK; }
int pstate_hash_dev(mina_ctx *, size_t n, size_t leg, HashLaunch hl, const uint32_t *, const uint32_t *d_nfields, uint32_t *, uint32_t *) {
    say("pstate_hash_dev", leg / MINA_STATES_PER_PROOF, ", %zu states of a leg of %zu, piece_waves %u (%zu states), lds %u", n, leg, hl.piece_waves, hash_piece_states(g_ctx, leg, hl.piece_waves), hl.lds_bytes);
    return marked(d_nfields) ? mb_fail(MINA_ERR_HIP, "state leg: marked") : MINA_OK;
}
int pstate_hash_dedup_dev(mina_ctx *, size_t n, size_t leg, HashLaunch hl, const uint32_t *, const uint32_t *d_nfields, uint32_t *, uint32_t *, bool count) {
    say("pstate_hash_dedup_dev", leg / MINA_STATES_PER_PROOF, ", %zu states of a leg of %zu, piece_waves %u, lds %u, count %d", n, leg, hl.piece_waves, hl.lds_bytes, (int)count);
    return marked(d_nfields) ? mb_fail(MINA_ERR_HIP, "state leg: marked") : MINA_OK;
}
void mb_launch_pstate_chain_check(hipStream_t st, uint32_t batch, const uint32_t *, const uint32_t *, const uint32_t *, const uint8_t *pre, uint32_t *) { say("mb_launch_pstate_chain_check", batch, " on s%d, precheck %d", mb_stub_id(st), pre ? 1 : 0); }
void mb_launch_fill_u32(hipStream_t st, uint32_t n, uint32_t v, uint32_t *) { say("mb_launch_fill_u32", n, " on s%d, value %u", mb_stub_id(st), v); }
void mb_launch_state_job_verdict(hipStream_t st, uint32_t batch, const uint32_t *, const uint32_t *ipa_v, const uint32_t *acc_v, const uint32_t *kimchi_bad, const uint32_t *stmt_ok, uint32_t *, uint32_t *flags, uint32_t *stmt_out) {
    say("mb_launch_state_job_verdict", batch, " on s%d, ipa %s acc %s kimchi_bad %s stmt_ok %s flags %d stmt_out %d", mb_stub_id(st), mb_stub_mem(ipa_v).c_str(), mb_stub_mem(acc_v).c_str(), mb_stub_mem(kimchi_bad).c_str(),
        mb_stub_mem(stmt_ok).c_str(), flags ? 1 : 0, stmt_out ? 1 : 0);
}
void mb_launch_challenge_to_field_fq(hipStream_t st, uint32_t n, FieldK, const uint32_t *, uint32_t *) { say("mb_launch_challenge_to_field_fq", n, " on s%d", mb_stub_id(st)); }
int mb_ipa_batch_check_dev(mina_ctx *, int curve, mb::IpaShape sh, const mb::IpaDevIn &in, uint32_t *, const FoldExport *fx) {
    say("mb_ipa_batch_check_dev", sh.batch, ", curve %d per %u override %d expand %d nshared %u export %d", curve, sh.per, (int)sh.override_slot, (int)sh.expand_slot, sh.nshared, fx ? 1 : 0);
    return marked(in.lr) ? mb_fail(MINA_ERR_HIP, "wrap-proof leg: marked") : MINA_OK;
}
int mb_accumulator_check_dev(mina_ctx *, int curve, uint32_t k, size_t batch, const uint32_t *d_prechal, const uint32_t *, const uint32_t *d_rho, uint32_t *, const FoldExport *fx) {
    say("mb_accumulator_check_dev", batch, ", curve %d k %u rho %d export %d", curve, k, d_rho ? 1 : 0, fx ? 1 : 0);
    return marked(d_prechal) ? mb_fail(MINA_ERR_HIP, "accumulator leg: marked") : MINA_OK;
}
namespace mb {
struct KimchiIn { const uint32_t *pub, *prev_chals, *prev_comms, *w_comm, *z_comm, *t_comm, *evals, *ft_eval1, *pubcomm; };
struct KimchiOut { uint32_t *sponge_state, *sponge_pos, *cip, *evalpoints, *polyscale, *evalscale, *comms, *ft_eval0; };
}
int mb_kimchi_to_batch_dev(mina_ctx *, size_t batch, uint32_t n_prev, uint32_t npub, const mb::KimchiIn &in, const mb::KimchiOut &, uint32_t *, mb::IpaExpand *, const void *pf_digest, uint32_t) {
    say("mb_kimchi_to_batch_dev", batch, ", n_prev %u npub %u pub %s prev_chals %s digest %d", n_prev, npub, mb_stub_mem(in.pub).c_str(), mb_stub_mem(in.prev_chals).c_str(), pf_digest ? 1 : 0);
    return MINA_OK;
}
int mb_pickles_statements_dev(mina_ctx *, size_t batch, const mina_pickles_statements *, uint32_t *, uint32_t *) { say("mb_pickles_statements_dev", batch); return MINA_OK; }
void mb_pickles_kimchi_digest(mina_ctx *, const mina_pickles_statements *s, const void **first, uint32_t *stride) { say("mb_pickles_kimchi_digest", 0); *first = s->sponge_digest; *stride = 32; }
int mb_pubcomm_dev(mina_ctx *, size_t batch, uint32_t log2_domain, uint32_t npub, const uint32_t *d_pub, uint32_t *) {
    say("mb_pubcomm_dev", batch, ", domain %u npub %u pub %s", log2_domain, npub, mb_stub_mem(d_pub).c_str());
    return MINA_OK;
}

// the context: mina_ctx_create / _set_pipeline / _pin_lane / _set_stream_budget / _synchronize / _destroy of api_core.hip, less everything installed
extern "C" int mina_ctx_create(int device_id, mina_ctx **out) {
    mina_ctx *c = new mina_ctx(); c->device = device_id;
    (void)hipStreamCreateWithFlags(&c->lanes[0].stream, hipStreamNonBlocking);
    c->use_lane0(); c->have_state_salts = true; *out = c; return MINA_OK;
}
extern "C" int mina_ctx_synchronize(mina_ctx *c) { return mb_ctx_wait_all(c) == hipSuccess ? MINA_OK : MINA_ERR_HIP; }
extern "C" void mina_ctx_destroy(mina_ctx *c) {
    for (int i = 0; i < MB_MAX_LANES; ++i) {
        Lane &L = c->lanes[i];
        if (L.ev_leg) (void)hipEventDestroy(L.ev_leg);
        if (L.ev_done) (void)hipEventDestroy(L.ev_done);
        if (L.stream && i < MB_DEV_HELPER0) (void)hipStreamDestroy(L.stream);
    }
    for (hipStream_t s : c->fork_own) if (s) (void)hipStreamDestroy(s);
    for (hipStream_t s : c->role) if (s) (void)hipStreamDestroy(s);
    delete c;
}
static mina_ctx *context(int lanes, int budget, int pinned = -1) {
    mina_ctx *c = nullptr; (void)mina_ctx_create(0, &c);
    for (int i = 1; i < lanes; ++i) (void)hipStreamCreateWithFlags(&c->lanes[i].stream, hipStreamNonBlocking);
    c->nlanes = lanes; c->stream_budget = budget; c->pinned = pinned;
    return g_ctx = c;
}
static void set_budget(mina_ctx *c, int n) { (void)mb_ctx_wait_all(c); c->stream_budget = n; }

// ------------------------------------------------------------------------------------------------ the jobs
// Every section of a job is a word of its own in `w` (the stubs read nothing but the markers); verdict and flag words in `out`.
struct Job {
    mina_state_jobs j; mina_kimchi_proofs kp; mina_pickles_statements st;
    uint32_t w[48]; std::vector<uint32_t> out;
    Job(const Job &) = delete;
    explicit Job(size_t batch, bool kimchi = true, bool statements = true) : out(2 * batch + 4) {
        memset(&j, 0, sizeof j); memset(&kp, 0, sizeof kp); memset(&st, 0, sizeof st); memset(w, 0, sizeof w);
        int at = 0; auto next = [&]() -> const void * { return &w[at++]; };
        j.batch = batch;
        j.with_states = 1; j.state_records = next(); j.state_nfields = next(); j.expected_hashes = next(); j.precheck = next();
        j.log2_domain = 15; j.npub = 40; j.public_inputs = next();
        j.with_ipa = 1; j.k = 15; j.n_evalpoints = 2; j.n_comms = 47;
        j.lr = next(); j.delta = next(); j.sg = next(); j.z1 = next(); j.z2 = next(); j.rand_base = next(); j.sg_rand_base = next();
        j.sponge_state = next(); j.sponge_pos = next(); j.cip = next(); j.evalpoints = next(); j.evalscale = next(); j.polyscale = next(); j.comms = next();
        j.with_accumulator = 1; j.acc_k = 16; j.acc_prechallenges = next(); j.acc_sg = next(); j.acc_rho = next();
        kp.batch = batch; kp.n_prev = 2; kp.npub = 40; kp.prev_comms = next(); kp.w_comm = next(); kp.z_comm = next(); kp.t_comm = next(); kp.evals = next(); kp.ft_eval1 = next();
        st.wrap_old_challenges = next(); st.sponge_digest = next();
        if (kimchi) j.kimchi = &kp;
        if (statements) kp.statements = &st;                         // the recursion challenges come from the statement
        else { kp.public_inputs = j.public_inputs; kp.prev_prechallenges = next(); }      // 128-bit prechallenges, expanded on the wrap leg's lane
    }
    uint32_t *verdicts() { return out.data(); }
    uint32_t *flags() { return out.data() + j.batch; }
    uint32_t *stmt() { return flags() + 4; }
    Job &fail_state() { *(uint32_t *)j.state_nfields = BAD; return *this; }
    Job &fail_wrap() { *(uint32_t *)j.lr = BAD; return *this; }
    Job &fail_acc() { *(uint32_t *)j.acc_prechallenges = BAD; return *this; }
};
static int g_errors = 0;
static void result(int rc, bool expect_failure = false) {
    if (rc) printf("-> error %d: %s\n", rc, mina_last_error());
    if ((rc != 0) != expect_failure) ++g_errors;
}
static void heading(const char *fmt, ...) { va_list ap; va_start(ap, fmt); printf("# "); vprintf(fmt, ap); printf("\n"); va_end(ap); }
static mina_verify_tuning tuned(void (*set)(mina_verify_tuning &)) { mina_verify_tuning t; mina_verify_tuning_default(&t); set(t); return t; }
// (device-resident jobs take the prepared rows: two stub lines per wrap-proof leg; the kimchi forms of the leg are the inline scenarios' and one of these)
static void dev_jobs(mina_ctx *c, int n, size_t batch = 3, bool kimchi = false) { for (int i = 0; i < n; ++i) { Job jb(batch, kimchi); jb.j.pub_comm_slot = 1; result(mina_state_job_batch_dev(c, &jb.j, jb.verdicts(), jb.flags())); } }
static void done(mina_ctx *c) { printf("mina_ctx_synchronize, mina_ctx_destroy\n"); (void)mina_ctx_synchronize(c); mina_ctx_destroy(c); g_ctx = nullptr; }

// ---- mb_state_jobs_on_lane as its callers in api_state.hip and api_verify.hip use it
static void inline_jobs() {
    mina_ctx *c = context(1, 0);
    auto run = [&](const char *what, Job &jb) { heading("inline job (StateJobPlan{}): %s", what); c->use_lane0(); result(mb_state_jobs_on_lane(c, &jb.j, jb.verdicts(), jb.flags())); };
    { Job jb(3); run("every section, kimchi from statements", jb); }
    { Job jb(3); jb.j.with_states = 0; jb.j.precheck = nullptr; run("with_states off", jb); }
    { Job jb(3); jb.j.with_states = 0; heading("inline job: with_states off but a precheck: an argument error"); c->use_lane0(); result(mb_state_jobs_on_lane(c, &jb.j, jb.verdicts(), jb.flags()), true); }
    { Job jb(3); jb.j.with_ipa = 0; jb.j.kimchi = nullptr; jb.j.npub = 0; run("with_ipa off, no public inputs", jb); }
    { Job jb(3); jb.j.with_ipa = 0; jb.j.kimchi = nullptr; run("with_ipa off, public-input commitment alone", jb); }
    { Job jb(3); jb.j.with_accumulator = 0; run("with_accumulator off", jb); }
    { Job jb(1); jb.j.acc_rho = nullptr; run("one proof, no acc_rho", jb); }
    { Job jb(3, false); jb.j.pub_comm_slot = 1; run("kimchi off: prepared rows, public-input commitment in slot 1", jb); }
    { Job jb(3, false); jb.j.npub = 0; run("kimchi off, no public inputs", jb); }
    { Job jb(3, true, false); run("kimchi without statements, prechallenges expanded", jb); }
    { Job jb(3, true, false); jb.kp.prev_prechallenges = nullptr; jb.kp.prev_chals = jb.j.comms; run("kimchi without statements, expanded challenges given", jb); }
    { Job jb(3); mina_verify_tuning t = tuned([](mina_verify_tuning &t) { t.kimchi_shared_digest = 0; t.ipa_shared_points = 0; }); mina_verify_configure_ex(&t); run("kimchi from statements, shared digest and shared points off", jb); mina_verify_configure_ex(nullptr); }
    { Job jb(3); (void)mb_ctx_state_dedup(c, true); run("mina_ctx_set_state_dedup on", jb); (void)mb_ctx_state_dedup(c, false); }
    heading("the three-lane plan of state_job_each (wrap = lanes[1], acc = lanes[2]), twice, then the states-only run of a culprit search");
    for (int i = 0; i < 2; ++i) { Job jb(4); StateJobPlan p; p.d_stmt_out = jb.stmt(); p.wrap = &c->lanes[1]; p.acc = &c->lanes[2]; c->use_lane0(); result(mb_state_jobs_on_lane(c, &jb.j, jb.verdicts(), jb.flags(), p)); }
    { Job jb(4); jb.j.with_ipa = 0; jb.j.with_accumulator = 0; jb.j.npub = 0; jb.j.kimchi = nullptr; c->use_lane0(); result(mb_state_jobs_on_lane(c, &jb.j, jb.verdicts(), jb.flags())); }
    done(c);
}

// the boundary: MB_JOB_LEGS, the early hashes of the records as they arrive, MB_JOB_FINISH with the carry (api_verify.hip issue_legs / stream_records / finish)
static void boundary_jobs(bool failing) {
    mina_ctx *c = context(1, 0);
    hipStream_t up = nullptr; hipEvent_t ev_up = nullptr;
    (void)hipStreamCreateWithFlags(&up, hipStreamNonBlocking); (void)hipEventCreateWithFlags(&ev_up, hipEventDisableTiming);
    const int slot = 1;
    Lane &L = c->lanes[slot], *h = &c->lanes[MB_PIPE_LANES + 3 * slot];
    (void)hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking);
    for (int q = 0; q < 3; ++q) (void)hipStreamCreateWithFlags(&h[q].stream, hipStreamNonBlocking);
    struct Triple { const char *name; Lane *wrap, *acc, *states; } triples[] = {{"(null, null, null)", nullptr, nullptr, nullptr}, {"(h, h + 1, h + 2)", &h[0], &h[1], &h[2]}, {"(h, h + 1, null)", &h[0], &h[1], nullptr}};
    const size_t B = 4, ns = B * MINA_STATES_PER_PROOF;
    if (failing) {
        heading("the boundary's lanes (h, h + 1, h + 2): the wrap-proof leg fails in MB_JOB_LEGS, then a whole good job");
        { Job jb(B); jb.fail_wrap(); StateJobCarry carry; StateJobPlan p; p.wrap = &h[0]; p.acc = &h[1]; p.states = &h[2]; p.phase = MB_JOB_LEGS; p.carry = &carry; c->L = &L; result(mb_state_jobs_on_lane(c, &jb.j, jb.verdicts(), jb.flags(), p), true); }
        heading("... the protocol-state leg fails in MB_JOB_FINISH");
        { Job jb(B); jb.fail_state(); StateJobCarry carry; StateJobPlan p; p.wrap = &h[0]; p.acc = &h[1]; p.states = &h[2]; p.carry = &carry; c->L = &L;
          p.phase = MB_JOB_LEGS; result(mb_state_jobs_on_lane(c, &jb.j, jb.verdicts(), jb.flags(), p));
          p.phase = MB_JOB_FINISH; result(mb_state_jobs_on_lane(c, &jb.j, jb.verdicts(), jb.flags(), p), true); }
    } else for (const Triple &t : triples) for (size_t early : {(size_t)0, (size_t)2 * MINA_STATES_PER_PROOF + 5, ns}) {
        heading("the boundary's two phases on lanes %s, %zu of %zu states hashed early", t.name, early, ns);
        Job jb(B); StateJobCarry carry;
        StateJobPlan p; p.wrap = t.wrap; p.acc = t.acc; p.states = t.states; p.carry = &carry; p.d_stmt_out = jb.stmt(); p.hash.piece_waves = 1024;
        c->L = &L; p.phase = MB_JOB_LEGS;
        result(mb_state_jobs_on_lane(c, &jb.j, jb.verdicts(), jb.flags(), p));
        c->use_lane0();
        if (early) {
            (void)hipEventRecord(ev_up, up);
            result(mb_state_hashes_early(c, t.states ? t.states : &L, ns, 0, early, (const uint32_t *)jb.j.state_records, (const uint32_t *)jb.j.state_nfields, ev_up, p.hash));
        }
        c->L = &L; p.phase = MB_JOB_FINISH; p.hashed_early = early;
        result(mb_state_jobs_on_lane(c, &jb.j, jb.verdicts(), jb.flags(), p));
        c->use_lane0();
    }
    if (!failing) {
        heading("mb_state_hashes_early: a range past the leg, no salts");
        result(mb_state_hashes_early(c, &L, ns, ns, 1, nullptr, nullptr, nullptr, HashLaunch{}), true);
        c->have_state_salts = false; result(mb_state_hashes_early(c, &L, ns, 0, 1, nullptr, nullptr, nullptr, HashLaunch{}), true); c->have_state_salts = true;
        heading("a split job without a carry");
        { Job jb(B); StateJobPlan p; p.phase = MB_JOB_LEGS; c->L = &L; result(mb_state_jobs_on_lane(c, &jb.j, jb.verdicts(), jb.flags(), p), true); }
    }
    for (int q = 0; q < 3; ++q) { (void)hipStreamDestroy(h[q].stream); h[q].stream = nullptr; }
    (void)hipStreamDestroy(up); (void)hipEventDestroy(ev_up);
    done(c);
}

// ---- mina_state_job_batch_dev / mina_state_job_fold_dev through dev_fork_lanes
static void device_jobs() {
    mina_ctx *c;
    heading("device-resident jobs: one lane, three jobs"); c = context(1, 3); dev_jobs(c, 3); done(c);
    heading("kimchi from statements: one lane, then 2 lanes at budget 3"); c = context(1, 3); dev_jobs(c, 1, 3, true); done(c); c = context(2, 3); dev_jobs(c, 1, 3, true); done(c);
    heading("a pinned lane (2) of a 4-lane context, two jobs, then unpinned at budget 3, then pinned again"); c = context(4, 3, 2); dev_jobs(c, 2); c->pinned = -1; dev_jobs(c, 4); c->pinned = 2; dev_jobs(c, 1); done(c);
    for (int budget : {23, 7, 3, 2, 1}) { heading("4 lanes at stream budget %d, %d jobs", budget, budget == 23 || budget == 3 ? 4 : 5); c = context(4, budget); dev_jobs(c, budget == 23 || budget == 3 ? 4 : 5); done(c); }
    heading("the environment's budget (GPU_MAX_HW_QUEUES = 4: 3 streams), 2 lanes"); c = context(2, 0); dev_jobs(c, 2); done(c);
    heading("9 lanes do not fork"); c = context(9, 23); dev_jobs(c, 2); done(c);
    for (uint32_t mode : {0u, 1u, 3u, 5u}) {
        mina_verify_tuning t; mina_verify_tuning_default(&t); t.dev_fork = mode; t.dev_chain_cus = 96; mina_verify_configure_ex(&t);
        heading("dev_fork = %u, dev_chain_cus 96: 2 lanes at budget 23 (plan A), 3 jobs", mode); c = context(2, 23); dev_jobs(c, 3); done(c);
        if (mode == 5u) { heading("dev_fork = 5: 2 lanes at budget 3 (plan B), 3 jobs"); c = context(2, 3); dev_jobs(c, 3); done(c); }
    }
    { mina_verify_tuning t = tuned([](mina_verify_tuning &t) { t.dev_fork = 3; t.dev_chain_cus = 0; }); mina_verify_configure_ex(&t); heading("dev_fork = 3, dev_chain_cus 0: no masks, one lane"); c = context(1, 23); dev_jobs(c, 1); done(c); }
    for (uint32_t al : {0u, 1u, 2u}) {
        mina_verify_tuning t; mina_verify_tuning_default(&t); t.dev_acc_lane = al; mina_verify_configure_ex(&t);
        heading("dev_acc_lane = %u: 2 lanes at budget 23, 2 jobs, then at budget 3, 2 jobs", al); c = context(2, 23); dev_jobs(c, 2); set_budget(c, 3); dev_jobs(c, 2); done(c);
    }
    for (uint32_t v : {0u, 512u, 0xffffffffu}) {
        mina_verify_tuning t; mina_verify_tuning_default(&t); t.dev_piece_waves = v; t.dev_hash_lds_kb = v == 512u ? 16u : v; mina_verify_configure_ex(&t);
        heading("dev_piece_waves = %u, dev_hash_lds_kb = %u: one lane, then 2 lanes at budget 23, then at budget 3", t.dev_piece_waves, t.dev_hash_lds_kb);
        c = context(1, 23); dev_jobs(c, 1); done(c); c = context(2, 23); dev_jobs(c, 1); set_budget(c, 3); dev_jobs(c, 1); done(c);
    }
    { mina_verify_tuning t = tuned([](mina_verify_tuning &t) { t.dev_hash_lds_kb = 200; }); mina_verify_configure_ex(&t); heading("dev_hash_lds_kb = 200: above the limit, none"); c = context(1, 23); dev_jobs(c, 1); done(c); }
    mina_verify_configure_ex(nullptr);
    heading("the piece arithmetic: 4 lanes at budget 23 with the single-lane rows installed, 963 and 964 proofs (4 x 17 x 964 >= HASH1_MIN_STATES), then without the rows");
    c = context(4, 23); c->pparams_rows1[FIELD_FP] = true; dev_jobs(c, 1, 963); dev_jobs(c, 1, 964); c->pparams_rows1[FIELD_FP] = false; dev_jobs(c, 1, 964); done(c);
    for (int budget : {23, 3}) { heading("13 jobs back to back over 4 lanes at budget %d", budget); c = context(4, budget); dev_jobs(c, 13); done(c); }
    heading("budgets 23 -> 3 -> 23 -> 3 on one 2-lane context, 2 jobs each: the lanes go from their own streams to the role streams and back"); c = context(2, 23); dev_jobs(c, 2); for (int budget : {3, 23, 3}) { set_budget(c, budget); dev_jobs(c, 2); } done(c);
    heading("mina_ctx_set_state_dedup on: one lane, then 4 lanes at budget 3"); c = context(1, 3); (void)mb_ctx_state_dedup(c, true); dev_jobs(c, 2); done(c); c = context(4, 3); (void)mb_ctx_state_dedup(c, true); dev_jobs(c, 2); done(c);
    heading("jobs without a protocol-state section, without an opening, without an accumulator: 2 lanes at budget 23, then at budget 3");
    c = context(2, 23);
    for (int pass = 0; pass < 2; ++pass) {
        { Job jb(2); jb.j.with_states = 0; jb.j.precheck = nullptr; result(mina_state_job_batch_dev(c, &jb.j, jb.verdicts(), jb.flags())); }
        { Job jb(2); jb.j.with_ipa = 0; jb.j.kimchi = nullptr; jb.j.npub = 0; result(mina_state_job_batch_dev(c, &jb.j, jb.verdicts(), nullptr)); }
        { Job jb(2); jb.j.with_accumulator = 0; result(mina_state_job_batch_dev(c, &jb.j, jb.verdicts(), jb.flags())); }
        set_budget(c, 3);
    }
    heading("argument errors of mina_state_job_batch_dev");
    { Job jb(2); result(mina_state_job_batch_dev(c, &jb.j, nullptr, nullptr), true); c->have_state_salts = false; result(mina_state_job_batch_dev(c, &jb.j, jb.verdicts(), nullptr), true); c->have_state_salts = true; }
    done(c);
    auto fold = [&](mina_ctx *c, int n) { for (int i = 0; i < n; ++i) { Job jb(3); uint32_t e[4]; result(mina_state_job_fold_dev(c, &jb.j, jb.verdicts(), jb.flags(), &e[0], &e[1], &e[2], &e[3])); } };
    heading("mina_state_job_fold_dev: one lane, two jobs"); c = context(1, 3); fold(c, 2); done(c);
    heading("mina_state_job_fold_dev: a pinned lane (1) of a 4-lane context"); c = context(4, 3, 1); fold(c, 2); done(c);
    heading("mina_state_job_fold_dev: 4 lanes at budget 3, 5 jobs"); c = context(4, 3); fold(c, 5); done(c);
    heading("mina_state_job_fold_dev: argument errors");
    c = context(1, 3);
    { Job jb(1); uint32_t e[4]; result(mina_state_job_fold_dev(c, &jb.j, jb.verdicts(), jb.flags(), &e[0], &e[1], &e[2], &e[3]), true); }
    { Job jb(3); uint32_t e[4]; result(mina_state_job_fold_dev(c, &jb.j, jb.verdicts(), jb.flags(), nullptr, &e[1], &e[2], &e[3]), true); }
    done(c);
}

// ---- a leg fails after the job has forked: what is queued is joined before the error returns (recorded AFTER the move: see the golden file's heading)
static void failing_jobs() {
    Job &(Job::*marks[3])() = {&Job::fail_state, &Job::fail_wrap, &Job::fail_acc};
    const char *names[3] = {"protocol-state", "wrap-proof", "accumulator"};
    for (int plan = 0; plan < 2; ++plan) for (int leg = 0; leg < 3; ++leg) {
        heading("the %s leg fails under plan %s: a good job, the failing one, mina_ctx_synchronize, a good job on every lane", names[leg], plan ? "B (4 lanes at budget 3; the failing job on lane 1)" : "A (one lane)");
        mina_ctx *c = context(plan ? 4 : 1, plan ? 3 : 23);
        dev_jobs(c, 1);
        { Job jb(3); (jb.*marks[leg])(); result(mina_state_job_batch_dev(c, &jb.j, jb.verdicts(), jb.flags()), true); }
        printf("mina_ctx_synchronize\n"); (void)mina_ctx_synchronize(c);
        dev_jobs(c, plan ? 4 : 1);
        done(c);
    }
    heading("the wrap-proof leg fails under plan B, then the lane is pinned: the next job runs under plan A behind the failed one");
    { mina_ctx *c = context(4, 3); Job jb(3); jb.fail_wrap(); result(mina_state_job_batch_dev(c, &jb.j, jb.verdicts(), jb.flags()), true); c->pinned = 0; dev_jobs(c, 1); done(c); }
    heading("the accumulator leg fails under the three-lane plan of state_job_each");
    { mina_ctx *c = context(1, 0); Job jb(4); jb.fail_acc(); StateJobPlan p; p.wrap = &c->lanes[1]; p.acc = &c->lanes[2]; c->use_lane0(); result(mb_state_jobs_on_lane(c, &jb.j, jb.verdicts(), jb.flags(), p), true); done(c); }
    boundary_jobs(true);
}

int main(int argc, char **argv) {
    setenv("GPU_MAX_HW_QUEUES", "4", 1);          // the budget of a context that sets none: 3 streams
    setvbuf(stdout, nullptr, _IOFBF, 1 << 16);
    inline_jobs();
    boundary_jobs(false);
    device_jobs();
    const bool moved = argc > 1 && !strcmp(argv[1], "moved");      // the part recorded where the functions had only been moved
    if (!moved) {
        heading("FAILURE PATHS (recorded after the scope guard: everything above was recorded at the commit that only moved the functions)");
        failing_jobs();
    }
    fflush(stdout);
    if (mb_stub_live_allocs()) { fprintf(stderr, "trace_state_job: %ld allocations still live after the last mina_ctx_destroy\n", mb_stub_live_allocs()); return 1; }
    if (moved) return g_errors ? 1 : 0;
    fprintf(stderr, "trace_state_job: %d unexpected results\n", g_errors);
    return g_errors ? 1 : 0;
}
