// api_core.hip -- context lifetime, field constants, field self-test hooks, K4 group map entry point.  (The host-only infrastructure -- error text, tuning, CSPRNG,
// worker pool -- lives in host_core.hip.)
#include "ctx.h"
#include "sponge.cuh"
#include "msm.cuh"

#include <sys/random.h>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <mutex>

// ------------------------------------------------------------------------------------------------
// Host-side derivation of the per-field constants (no table of magic numbers: everything follows
// from the modulus and the generator 5).
template <int F> static fe_t host_modulus() { fe_t p; for (int i = 0; i < 8; ++i) p.v[i] = modulus_limb<F>(i); return p; }
static void fe_shr1(fe_t &a) { for (int i = 0; i < 7; ++i) a.v[i] = (a.v[i] >> 1) | (a.v[i + 1] << 31); a.v[7] >>= 1; }
static fe_t fe_sub_small(const fe_t &a, uint32_t k) { fe_t r = a; uint64_t br = k; for (int i = 0; i < 8 && br; ++i) { uint64_t t = (uint64_t)r.v[i] - br; r.v[i] = (uint32_t)t; br = (t >> 32) & 1u; } return r; }
static fe_t fe_div3(const fe_t &a) { fe_t r; uint64_t rem = 0; for (int i = 7; i >= 0; --i) { uint64_t cur = (rem << 32) | a.v[i]; r.v[i] = (uint32_t)(cur / 3); rem = cur % 3; } return r; }

template <int F> static FieldK make_field_consts() {
    FieldK k;
    fe_t p = host_modulus<F>();
    // R mod p and R^2 mod p by modular doubling of 1 (fe_add works on any residues)
    fe_t a = fe_zero(); a.v[0] = 1;
    for (int i = 0; i < 512; ++i) { a = fe_add<F>(a, a); if (i == 255) k.one = a; }
    k.r2 = a;
    fe_t pm1 = fe_sub_small(p, 1);
    k.pm2 = fe_sub_small(p, 2);
    k.pm1d2 = pm1; fe_shr1(k.pm1d2);
    k.half = k.pm1d2;
    fe_t t = pm1; for (int i = 0; i < 32; ++i) fe_shr1(t);
    k.tm1d2 = fe_sub_small(t, 1); fe_shr1(k.tm1d2);
    fe_t five = fe_zero(); five.v[0] = 5; k.five = fe_to_mont<F>(five, k.r2);
    k.root = fe_pow<F>(k.five, t, k.one);
    fe_t three = fe_zero(); three.v[0] = 3; three = fe_to_mont<F>(three, k.r2);
    fe_t six = fe_zero(); six.v[0] = 6; k.bw_fu = fe_to_mont<F>(six, k.r2);
    fe_t two = fe_dbl<F>(k.one);
    fe_sqrt<F>(k.bw_s, fe_neg<F>(three), k);
    k.bw_c = fe_mul<F>(fe_sub<F>(k.bw_s, k.one), fe_inv<F>(two, k));
    k.bw_inv3 = fe_inv<F>(three, k);
    fe_t w = fe_pow<F>(k.five, fe_div3(pm1), k.one);
    k.endo = fe_sqr<F>(w);
    k.inv2 = fe_inv<F>(two, k);
    k.two255 = k.one; for (int i = 0; i < 255; ++i) k.two255 = fe_dbl<F>(k.two255);
    { fe_t t = fe_zero(); t.v[0] = 32; k.m32 = fe_to_mont<F>(t, k.r2); }
    return k;
}

// ------------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------------

extern "C" int mina_ctx_create(int device_id, mina_ctx **out) {
    if (!out) return fail(MINA_ERR_ARG, "out is null");
    *out = nullptr;
    int ndev = 0;
    HIPC(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail(MINA_ERR_HIP, "no HIP device: libminaverify has no CPU fallback");
    if (device_id < 0 || device_id >= ndev) return fail(MINA_ERR_ARG, "bad device id");
    HIPC(hipSetDevice(device_id));
    mina_ctx *c = new mina_ctx();
    c->device = device_id;
    hipError_t e = hipStreamCreateWithFlags(&c->lanes[0].stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return fail(MINA_ERR_HIP, "hipStreamCreate failed"); }
    c->use_lane0();
    c->fk[FIELD_FP] = make_field_consts<FIELD_FP>();
    c->fk[FIELD_FQ] = make_field_consts<FIELD_FQ>();
    c->state_frontend = mb_state_frontend_on_lane;
    c->account_on_device = mb_verify_account_dev_on;
    c->state_job_each = mb_state_job_each_host;
    c->state_job_checks = mb_state_job_checks_host;
    c->pickles_statements_net = mb_pickles_statements_net_dev;
    c->kimchi_to_batch_net = mb_kimchi_to_batch_net_dev;
    c->mixed_sets_check = mb_mixed_sets_check;
    c->state_job_each_net = mb_state_job_each_net_host;
    *out = c;
    return MINA_OK;
}

int mb_ctx_create_view(mina_ctx *parent, mina_ctx **out) {
    if (!parent || !out) return fail(MINA_ERR_ARG, "null argument");
    int rc = mina_ctx_create(parent->device, out);
    if (rc) return rc;
    (*out)->is_view = true;
    mb_ctx_refresh_view(*out, parent);
    return MINA_OK;
}

extern "C" void mina_ctx_destroy(mina_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (int i = 0; i < MB_DEV_HELPER0; ++i) if (c->lanes[i].stream) (void)hipStreamSynchronize(c->lanes[i].stream);
    for (hipStream_t s : c->fork_own) if (s) (void)hipStreamSynchronize(s);
    for (hipStream_t s : c->role) if (s) (void)hipStreamSynchronize(s);
    c->free_step_host(); c->parked.free_step_host();
    for (auto &r : c->prof.recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (int i = 0; i < MB_MAX_LANES; ++i) {
        Lane &L = c->lanes[i];
        if (L.aux) { (void)hipStreamSynchronize(L.aux); (void)hipStreamDestroy(L.aux); (void)hipEventDestroy(L.ev_fork); (void)hipEventDestroy(L.ev_join); }
        if (L.ev_leg) (void)hipEventDestroy(L.ev_leg);
        if (L.ev_done) (void)hipEventDestroy(L.ev_done);
        if (L.stream && i < MB_DEV_HELPER0) (void)hipStreamDestroy(L.stream);      // (the helper lanes of the forked jobs alias the streams below)
    }
    for (hipStream_t s : c->fork_own) if (s) (void)hipStreamDestroy(s);
    for (hipStream_t s : c->role) if (s) (void)hipStreamDestroy(s);
    delete c;
}

// The lanes of a context (and the concurrent culprit search of mina_state_job_batch) are separate streams; they only run side by side
// on separate hardware queues, and the runtime's default is 4.  The HIP runtime reads the variable when it initialises, so this takes
// effect when the library is loaded before the process's first HIP call (the operator's cgo binding); a value set by the user is kept.
// 16: what the reference-shaped boundary wants -- a lone job's three legs + the other slots; measured with the system runtime (ROCm 7.2), 8192
// proofs per mina_verify_state_batch call: 4 - 16 queues 54.6 - 56 ms, 24 queues 68.4 ms.  A process that pipelines device-resident jobs
// itself (bench.py's headline: 4 lanes x 4 streams since round 6; the test-suite) sets 24 -- one queue per stream plus a few; a process should never hold more streams than that.
__attribute__((constructor)) static void mb_default_hw_queues() { setenv("GPU_MAX_HW_QUEUES", "16", 0); }

// The index set (0 | 1) every installer, loader, getter and job of the context acts on (ctx.h IndexSet).  Host bookkeeping only: no HIP call, no allocation, no
// synchronisation; launches already queued keep the buffers they captured.  Like an install, not to be called while another thread queues work on the context.
extern "C" int mina_ctx_select_index_set(mina_ctx *c, uint32_t set) {
    if (!c) return fail(MINA_ERR_ARG, "null ctx");
    if (set > 1) return fail(MINA_ERR_ARG, "index set: 0 or 1");
    c->select_index_set(set);
    return MINA_OK;
}
extern "C" uint32_t mina_ctx_index_set(const mina_ctx *c) { return c ? c->index_set : 0; }
extern "C" int mina_ctx_mixed_job_stats(mina_ctx *c, uint64_t *jobs, uint64_t *proofs_set0, uint64_t *proofs_set1) {
    if (!c || !jobs || !proofs_set0 || !proofs_set1) return fail(MINA_ERR_ARG, "null argument");
    uint64_t tot[2] = {0, 0};
    if (c->mixed_totals.p) {                                    // summed on the device: behind everything the context has queued
        HIPC(hipSetDevice(c->device));
        HIPC(mb_ctx_wait_all(c));
        HIPC(hipMemcpy(tot, c->mixed_totals.p, sizeof tot, hipMemcpyDeviceToHost));
    }
    *jobs = c->mixed_jobs; *proofs_set0 = tot[0]; *proofs_set1 = tot[1];
    return MINA_OK;
}

extern "C" int mina_ctx_synchronize(mina_ctx *c) {
    if (!c) return fail(MINA_ERR_ARG, "null ctx");
    HIPC(hipSetDevice(c->device));
    HIPC(mb_ctx_wait_all(c));
    return MINA_OK;
}
// The streams the forked device-resident jobs of this context may keep busy (ctx.h stream_plan): n <= 0 = what the environment gives (GPU_MAX_HW_QUEUES less the
// caller's null stream).  Tests and tools force a plan with it; waits for what is queued, so that the next job may flow through other streams.
extern "C" int mina_ctx_set_stream_budget(mina_ctx *c, int n) {
    if (!c) return fail(MINA_ERR_ARG, "null ctx");
    if (n > 31) return fail(MINA_ERR_ARG, "stream budget: at most 31 (32 hardware queues less the null stream's); <= 0 = the environment's");
    HIPC(hipSetDevice(c->device));
    HIPC(mb_ctx_wait_all(c));
    c->stream_budget = n > 0 ? n : 0;
    return MINA_OK;
}
// The plan the context's last forked device-resident job was queued under (ctx.h StreamPlan; state_job.hip dev_fork_lanes): all zero under plan A and before the first job
extern "C" int mina_ctx_stream_plan_stats(mina_ctx *c, uint32_t *roles, uint32_t *carriers, uint32_t *sets, uint32_t *streams) {
    if (!c || !roles || !carriers || !sets || !streams) return fail(MINA_ERR_ARG, "null argument");
    const StreamPlan &p = c->last_plan;
    *roles = p.roles ? 1u : 0u; *carriers = (uint32_t)p.carriers; *sets = (uint32_t)p.sets; *streams = (uint32_t)p.busy();
    return MINA_OK;
}
extern "C" void *mina_ctx_stream(mina_ctx *c) { return c ? (void *)c->lanes[c->pinned >= 0 ? c->pinned : 0].stream : nullptr; }
// Pin the `_dev` entry points to ONE pipeline lane (lane < 0: back to round-robin).  While pinned, everything they queue is ordered on mina_ctx_stream(): a caller
// that queues its own kernels, copies and collectives on that stream (torch: ExternalStream) is ordered against the library by the stream itself -- no
// hipDeviceSynchronize between the steps of a multi-GPU exchange (mina_bridge_amd/sharded.py ShardedStateJob).
extern "C" int mina_ctx_pin_lane(mina_ctx *c, int lane) {
    if (!c) return fail(MINA_ERR_ARG, "null ctx");
    if (lane >= c->nlanes) return fail(MINA_ERR_ARG, "lane outside the pipeline (mina_ctx_set_pipeline)");
    c->pinned = lane < 0 ? -1 : lane;
    return MINA_OK;
}

extern "C" int mina_ctx_set_pipeline(mina_ctx *c, int lanes) {
    if (!c) return fail(MINA_ERR_ARG, "null ctx");
    if (lanes < 1 || lanes > MB_PIPE_LANES) return fail(MINA_ERR_ARG, "lanes must be in 1..32");
    HIPC(hipSetDevice(c->device));
    HIPC(mb_ctx_wait_all(c));
    for (int i = 0; i < lanes; ++i)
        if (!c->lanes[i].stream) HIPC(hipStreamCreateWithFlags(&c->lanes[i].stream, hipStreamNonBlocking));
    c->nlanes = lanes; c->rr = 0; c->pinned = -1; c->use_lane0();
    return MINA_OK;
}

// ------------------------------------------------------------------------------------------------
extern "C" int mina_to_group(mina_ctx *c, int curve, size_t n, const uint8_t *t, uint8_t *out) {
    if (!c || (n && (!t || !out))) return fail(MINA_ERR_ARG, "null argument");
    if (curve != 0 && curve != 1) return fail(MINA_ERR_ARG, "bad curve");
    if (n == 0) return MINA_OK;
    HIPC(hipSetDevice(c->device));
    c->use_lane0();
    int rc;
    if ((rc = h2d(c, c->L->tmp_a, t, n * 32))) return rc;
    if ((rc = c->L->tmp_b.ensure(n * 64))) return rc;
    const int F = base_field_of(curve);
    DISPATCH_FIELD(F, { to_group_kernel<F_><<<cdiv(n, 128), 128, 0, c->L->stream>>>((uint32_t)n, c->fk[F_], c->L->tmp_a.as<uint32_t>(), c->L->tmp_b.as<uint32_t>()); });
    return d2h_sync(c, out, c->L->tmp_b, n * 64);
}

extern "C" int mina_field_mul(mina_ctx *c, int field, size_t n, const uint8_t *a, const uint8_t *b, uint8_t *out) {
    if (!c || (n && (!a || !b || !out))) return fail(MINA_ERR_ARG, "null argument");
    if (bad_field(field)) return fail(MINA_ERR_ARG, "bad field");
    if (n == 0) return MINA_OK;
    HIPC(hipSetDevice(c->device));
    c->use_lane0();
    int rc;
    if ((rc = h2d(c, c->L->tmp_a, a, n * 32))) return rc;
    if ((rc = h2d(c, c->L->tmp_b, b, n * 32))) return rc;
    if ((rc = c->L->tmp_c.ensure(n * 32))) return rc;
    DISPATCH_FIELD(field, { field_mul_kernel<F_><<<cdiv(n, 256), 256, 0, c->L->stream>>>((uint32_t)n, c->fk[F_], c->L->tmp_a.as<uint32_t>(), c->L->tmp_b.as<uint32_t>(), c->L->tmp_c.as<uint32_t>()); });
    return d2h_sync(c, out, c->L->tmp_c, n * 32);
}
extern "C" int mina_field_inv(mina_ctx *c, int field, size_t n, const uint8_t *a, uint8_t *out) {
    if (!c || (n && (!a || !out))) return fail(MINA_ERR_ARG, "null argument");
    if (bad_field(field)) return fail(MINA_ERR_ARG, "bad field");
    if (n == 0) return MINA_OK;
    HIPC(hipSetDevice(c->device));
    c->use_lane0();
    int rc;
    if ((rc = h2d(c, c->L->tmp_a, a, n * 32))) return rc;
    if ((rc = c->L->tmp_c.ensure(n * 32))) return rc;
    DISPATCH_FIELD(field, { field_inv_kernel<F_><<<cdiv(n, 256), 256, 0, c->L->stream>>>((uint32_t)n, c->fk[F_], c->L->tmp_a.as<uint32_t>(), c->L->tmp_c.as<uint32_t>()); });
    return d2h_sync(c, out, c->L->tmp_c, n * 32);
}
// mina_field_inv on the divstep inversion (fe_modinv.cuh), whatever mina_ctx_set_fast_inverse says: the same arguments, errors and bytes
extern "C" int mina_field_inv_gcd(mina_ctx *c, int field, size_t n, const uint8_t *a, uint8_t *out) {
    if (!c || (n && (!a || !out))) return fail(MINA_ERR_ARG, "null argument");
    if (bad_field(field)) return fail(MINA_ERR_ARG, "bad field");
    if (n == 0) return MINA_OK;
    HIPC(hipSetDevice(c->device));
    c->use_lane0();
    int rc;
    if ((rc = h2d(c, c->L->tmp_a, a, n * 32))) return rc;
    if ((rc = c->L->tmp_c.ensure(n * 32))) return rc;
    DISPATCH_FIELD(field, { field_inv_gcd_kernel<F_><<<cdiv(n, 256), 256, 0, c->L->stream>>>((uint32_t)n, c->fk[F_], c->L->tmp_a.as<uint32_t>(), c->L->tmp_c.as<uint32_t>()); });
    return d2h_sync(c, out, c->L->tmp_c, n * 32);
}
extern "C" int mina_field_sqrt(mina_ctx *c, int field, size_t n, const uint8_t *a, uint8_t *out, uint8_t *ok) {
    if (!c || (n && (!a || !out || !ok))) return fail(MINA_ERR_ARG, "null argument");
    if (bad_field(field)) return fail(MINA_ERR_ARG, "bad field");
    if (n == 0) return MINA_OK;
    HIPC(hipSetDevice(c->device));
    c->use_lane0();
    int rc;
    if ((rc = h2d(c, c->L->tmp_a, a, n * 32))) return rc;
    if ((rc = c->L->tmp_c.ensure(n * 32))) return rc;
    if ((rc = c->L->tmp_d.ensure(n))) return rc;
    DISPATCH_FIELD(field, { field_sqrt_kernel<F_><<<cdiv(n, 256), 256, 0, c->L->stream>>>((uint32_t)n, c->fk[F_], c->L->tmp_a.as<uint32_t>(), c->L->tmp_c.as<uint32_t>(), c->L->tmp_d.as<uint8_t>()); });
    HIPC(hipMemcpyAsync(ok, c->L->tmp_d.p, n, hipMemcpyDeviceToHost, c->L->stream));
    return d2h_sync(c, out, c->L->tmp_c, n * 32);
}


// ------------------------------------------------------------------------------------------------
// stage timing
static const char *PROF_NAMES[PS_COUNT] = {"msm_digits", "msm_scan", "msm_scatter", "msm_accumulate", "msm_bucket_sum", "msm_segsum",
                                           "msm_reduce2d", "msm_finish", "bpoly_tables", "bpoly_fold", "bpoly_finish", "pstate_hash", "ipa_transcript", "kimchi_to_batch", "pickles_statement",
                                           "pstate_hash1"};
void mb_prof_begin(mina_ctx *c, int stage) {
    ProfState &p = c->prof;
    if (p.used == p.recs.size()) {
        ProfState::Rec r; r.stage = stage;
        if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return;
        p.recs.push_back(r);
    }
    p.recs[p.used].stage = stage;
    (void)hipEventRecord(p.recs[p.used].a, c->L->stream);
}
void mb_prof_end(mina_ctx *c, int stage) {
    ProfState &p = c->prof;
    if (p.used >= p.recs.size() || p.recs[p.used].stage != stage) return;
    (void)hipEventRecord(p.recs[p.used].b, c->L->stream);
    ++p.used;
}
extern "C" int mina_prof_enable(mina_ctx *c, int stage_mask) {
    if (!c) return fail(MINA_ERR_ARG, "null ctx");
    c->prof.mask = stage_mask; c->prof.used = 0;
    return MINA_OK;
}
// Synchronises the stream, writes {"stage": [launches, total_ms], ...} for everything recorded since the last
// read / enable, and resets the recording.
extern "C" int mina_prof_read(mina_ctx *c, char *buf, size_t cap) {
    if (!c || !buf || cap < 8) return fail(MINA_ERR_ARG, "bad argument");
    HIPC(hipSetDevice(c->device));
    HIPC(mb_ctx_wait_all(c));
    double tot[PS_COUNT] = {0}; int cnt[PS_COUNT] = {0};
    for (size_t i = 0; i < c->prof.used; ++i) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->prof.recs[i].a, c->prof.recs[i].b) == hipSuccess) { tot[c->prof.recs[i].stage] += ms; cnt[c->prof.recs[i].stage]++; }
    }
    c->prof.used = 0;
    std::string o = "{";
    bool first = true;
    for (int s = 0; s < PS_COUNT; ++s) {
        if (!cnt[s]) continue;
        char tmp[128]; snprintf(tmp, sizeof tmp, "%s\"%s\": [%d, %.6f]", first ? "" : ", ", PROF_NAMES[s], cnt[s], tot[s]);
        o += tmp; first = false;
    }
    o += "}";
    if (o.size() + 1 > cap) return fail(MINA_ERR_ARG, "buffer too small");
    memcpy(buf, o.c_str(), o.size() + 1);
    return MINA_OK;
}

// ------------------------------------------------------------------------------------------------
// self-test hook for the lane-cooperative group law: for each i runs the same chain of XYZZ operations
//   acc = P_i + Q_i; acc += acc (doubling branch); acc += Q_i; acc = 2*acc; acc += (-acc_before) ...
// once with the single-lane routines and once with the 4-lane cooperative ones; outputs both results (affine,
// canonical) and whether the XYZZ coordinates agreed word for word at every step.
template <int F>
__global__ void __launch_bounds__(256)
group_law_selftest_kernel(uint32_t n, FieldK fk, const uint32_t *__restrict__ pw, const uint32_t *__restrict__ qw,
                          uint32_t *__restrict__ out_serial, uint32_t *__restrict__ out_quad, uint32_t *__restrict__ same) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x, i = gid >> 2, rho = gid & 3;
    const bool live = i < n; const uint32_t ii = live ? i : 0;
    auto ld = [&](const uint32_t *w) { affine_t a; for (int k = 0; k < 8; ++k) { a.x.v[k] = w[(size_t)ii * 16 + k]; a.y.v[k] = w[(size_t)ii * 16 + 8 + k]; }
                                       a.x = fe_to_mont<F>(a.x, fk.r2); a.y = fe_to_mont<F>(a.y, fk.r2); return a; };
    const affine_t P = ld(pw), Q = ld(qw);
    const xyzz_t xp = xyzz_from_affine<F>(P, fk.one), xq = xyzz_from_affine<F>(Q, fk.one);
    auto eq = [](const xyzz_t &a, const xyzz_t &b) { return fe_eq(a.x, b.x) && fe_eq(a.y, b.y) && fe_eq(a.zz, b.zz) && fe_eq(a.zzz, b.zzz); };
    xyzz_t s = xp, c = xp; bool ok = true;
    xyzz_add<F>(s, xq);            xyzz_add_quad<F>(c, xq);            ok &= eq(s, c);
    { xyzz_t t = s; xyzz_add<F>(s, t); t = c; xyzz_add_quad<F>(c, t); } ok &= eq(s, c);      // P == Q branch
    xyzz_add<F>(s, xq);            xyzz_add_quad<F>(c, xq);            ok &= eq(s, c);
    s = xyzz_dbl<F>(s);            c = xyzz_dbl_quad<F>(c);            ok &= eq(s, c);
    { xyzz_t t = s; xyzz_add<F>(t, xp); xyzz_t u = c; xyzz_add_quad<F>(u, xp);                // general add with non-trivial ZZ on both sides
      xyzz_add<F>(s, t); xyzz_add_quad<F>(c, u); } ok &= eq(s, c);
    { xyzz_t t = s; t.y = fe_neg<F>(t.y); xyzz_t z = s; xyzz_add<F>(z, t); xyzz_t u = c; u.y = fe_neg<F>(u.y); xyzz_t z2 = c; xyzz_add_quad<F>(z2, u);
      ok &= xyzz_is_inf(z) && xyzz_is_inf(z2); }                                              // P == -Q branch
    auto st = [&](const xyzz_t &t, uint32_t *o) {
        if (xyzz_is_inf(t)) { for (int k = 0; k < 16; ++k) o[(size_t)i * 16 + k] = 0; return; }
        fe_t zi = fe_inv<F>(fe_mul<F>(t.zz, t.zzz), fk);
        fe_t x = fe_from_mont<F>(fe_mul<F>(t.x, fe_mul<F>(zi, t.zzz))), y = fe_from_mont<F>(fe_mul<F>(t.y, fe_mul<F>(zi, t.zz)));
        for (int k = 0; k < 8; ++k) { o[(size_t)i * 16 + k] = x.v[k]; o[(size_t)i * 16 + 8 + k] = y.v[k]; } };
    if (live && rho == 0) { st(s, out_serial); st(c, out_quad); same[i] = ok ? 1u : 0u; }
}

extern "C" int mina_selftest_group_law(mina_ctx *c, int curve, size_t n, const uint8_t *p, const uint8_t *q, uint8_t *out_serial,
                                       uint8_t *out_quad, uint8_t *same) {
    if (!c || (n && (!p || !q || !out_serial || !out_quad || !same))) return fail(MINA_ERR_ARG, "null argument");
    if (curve != 0 && curve != 1) return fail(MINA_ERR_ARG, "bad curve");
    if (n == 0) return MINA_OK;
    HIPC(hipSetDevice(c->device));
    c->use_lane0();
    int rc;
    if ((rc = h2d(c, c->L->tmp_a, p, n * 64))) return rc;
    if ((rc = h2d(c, c->L->tmp_b, q, n * 64))) return rc;
    if ((rc = c->L->tmp_c.ensure(n * 64))) return rc;
    if ((rc = c->L->tmp_d.ensure(n * 64 + n * 4))) return rc;
    uint32_t *d_quad = c->L->tmp_d.as<uint32_t>(), *d_same = d_quad + n * 16;
    DISPATCH_FIELD(base_field_of(curve), {
        group_law_selftest_kernel<F_><<<cdiv(n * 4, 256), 256, 0, c->L->stream>>>((uint32_t)n, c->fk[F_], c->L->tmp_a.as<uint32_t>(), c->L->tmp_b.as<uint32_t>(),
                                                                              c->L->tmp_c.as<uint32_t>(), d_quad, d_same);
    });
    std::vector<uint32_t> sm(n);
    HIPC(hipMemcpyAsync(out_quad, d_quad, n * 64, hipMemcpyDeviceToHost, c->L->stream));
    HIPC(hipMemcpyAsync(sm.data(), d_same, n * 4, hipMemcpyDeviceToHost, c->L->stream));
    if ((rc = d2h_sync(c, out_serial, c->L->tmp_c, n * 64))) return rc;
    for (size_t i = 0; i < n; ++i) same[i] = sm[i] ? 1 : 0;
    return MINA_OK;
}

// ------------------------------------------------------------------------------------------------
// plain device-memory helpers for callers of the `_dev` entry points that have no HIP binding of their own
extern "C" int mina_dev_malloc(mina_ctx *c, size_t bytes, void **out) {
    if (!c || !out) return fail(MINA_ERR_ARG, "null argument");
    *out = nullptr;
    HIPC(hipSetDevice(c->device));
    if (hipMalloc(out, bytes ? bytes : 4) != hipSuccess) return fail(MINA_ERR_HIP, "hipMalloc failed");
    return MINA_OK;
}
extern "C" int mina_dev_free(mina_ctx *c, void *p) {
    if (!c) return fail(MINA_ERR_ARG, "null argument");
    HIPC(hipSetDevice(c->device));
    if (p) HIPC(hipFree(p));
    return MINA_OK;
}
// synchronous copies (they wait for the context's lanes first, so results of queued `_dev` calls are visible)
extern "C" int mina_dev_upload(mina_ctx *c, void *dst, const void *src, size_t bytes) {
    if (!c || (bytes && (!dst || !src))) return fail(MINA_ERR_ARG, "null argument");
    HIPC(hipSetDevice(c->device));
    if (bytes) HIPC(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return MINA_OK;
}
extern "C" int mina_dev_download(mina_ctx *c, void *dst, const void *src, size_t bytes) {
    if (!c || (bytes && (!dst || !src))) return fail(MINA_ERR_ARG, "null argument");
    int rc = mina_ctx_synchronize(c);
    if (rc) return rc;
    if (bytes) HIPC(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return MINA_OK;
}
