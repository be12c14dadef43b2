// ctx.h -- shared host-side state of libminaverify.so (one mina_ctx = one GPU).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <array>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <algorithm>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/mina_verify.h"
#include "groupmap.cuh"

using namespace mb;

struct mina_ctx;
namespace mb { struct KimchiIn; struct KimchiOut; }   // api_kimchi.hip (state_job.hip restates them)
// A VIEW of a context (round 5): its own lanes, streams and workspaces, while everything INSTALLED -- field constants, both SRS with their window tables, Poseidon
// tables, salts, verifier / step index -- is borrowed from the parent (no second copy of the tables).  The boundary runs the culprit search of a failed chunk on a
// view, so that the search needs neither the parent's lock nor a drained device (api_verify.hip Device::sc).  mb_ctx_refresh_view (below mina_ctx) re-reads the
// parent's installs; the caller holds whatever serialises installs on the parent.  Destroy the view BEFORE the parent.
int mb_ctx_create_view(mina_ctx *parent, mina_ctx **out);
int mb_fail(int code, const std::string &msg);      // records the thread-local error text, returns code
mina_verify_tuning mb_tune();                        // the process-wide tuning (api_core.hip; mina_verify_configure_ex), by value
#define fail mb_fail

#define HIPC(expr)                                                                                 \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess)                                                                     \
            return fail(MINA_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));         \
    } while (0)

// Device memory (DevBuf) and page-locked host memory (PinnedBuf) that free themselves: whatever holds one by value needs no teardown list.  Two rules:
//   NO STATIC-STORAGE OBJECTS.  An object with static storage duration never holds one by value: its destructor would call into the runtime after the runtime has
//     shut down at process exit.  Every holder is a heap object (new mina_ctx, the boundary's new Device) or a local.
//   VIEW BEFORE PARENT.  A view context (Installed::borrow_from) is destroyed before the context it borrows from.
struct DevBuf {
    void *p = nullptr; size_t cap = 0;
    bool borrowed = false;             // the memory belongs to another context's DevBuf (a VIEW context: Installed::borrow_from): never freed here; outgrown -> replaced by an own allocation
    DevBuf() = default; DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete; ~DevBuf() { release(); }
    int ensure(size_t bytes) {
        if (bytes <= cap) return MINA_OK;
        if (p) { if (!borrowed && hipFree(p) != hipSuccess) return MINA_ERR_HIP; p = nullptr; cap = 0; borrowed = false; }
        size_t want = bytes + bytes / 8 + 256;
        if (hipMalloc(&p, want) != hipSuccess) return fail(MINA_ERR_HIP, "hipMalloc failed");
        cap = want; return MINA_OK;
    }
    void release() { if (p && !borrowed) (void)hipFree(p); p = nullptr; cap = 0; borrowed = false; }
    void alias(const DevBuf &o) { release(); p = o.p; cap = o.cap; borrowed = o.p != nullptr; }
    void swap(DevBuf &o) { std::swap(p, o.p); std::swap(cap, o.cap); std::swap(borrowed, o.borrowed); }   // the two handles change places; nothing is allocated or freed
    template <class T> T *as() { return reinterpret_cast<T *>(p); }
};

// page-locked host staging (grow-only): packing straight into it makes the H2D copy a real DMA at PCIe speed
struct PinnedBuf {
    void *p = nullptr; size_t cap = 0;
    PinnedBuf() = default; PinnedBuf(const PinnedBuf &) = delete; PinnedBuf &operator=(const PinnedBuf &) = delete; ~PinnedBuf() { release(); }
    int ensure(size_t bytes) {
        if (bytes <= cap) return MINA_OK;
        if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 4 + 4096;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) return fail(MINA_ERR_HIP, "hipHostMalloc failed");
        cap = want; return MINA_OK;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

struct SrsState {
    uint32_t depth = 0;
    uint32_t c = 16, W = 16;           // fixed-base window shape
    DevBuf table;                      // W * depth affine_t; window 0 = g itself
    DevBuf table29;                    // the same points with coordinates x * 2^261 mod p (8 x 32-bit words): what the fp29 accumulate kernels gather (ec29.cuh)
    DevBuf table29s;                   // ... pre-split: x, y, p - y as 9 x 29-bit limbs + an infinity flag, 128 B per point (msm.cuh tab29_t; mina_verify_tuning.msm_fp29 = 2)
    DevBuf h;                          // 1 affine_t
    int lagrange_log2 = -1;            // cached Lagrange basis (canonical affine bytes, host side)
    std::vector<uint8_t> lagrange_host;
    uint64_t srs_gen = 0;              // process-unique stamp of the SRS these tables were built from (api_srs.hip srs_alloc): a view context re-copies what it derived on a change
    DevBuf lagrange_table;             // window table (c = 8, W = 32) of the first lagrange_table_n basis points, for
    uint32_t lagrange_table_n = 0;     //   batched public-input commitments
    int lagrange_table_log2 = -1;
    DevBuf lagrange_digits;            // d * 2^(8w) * L_i, d = 1..128, of the first lagrange_digits_n (<= 64) basis points (lagrange.cuh: direct commitments)
    uint32_t lagrange_digits_n = 0;
    DevBuf lagrange_digits29;          // ... its 2^261-domain twin: the direct commitments' mixed adds run on 29-bit limbs (lagrange.cuh pubcomm_direct29_kernel)
    inline void borrow_from(const SrsState &b) {    // a view context's (Installed::borrow_from): every field above, the tables aliased
        SrsState &a = *this;
        a.depth = b.depth; a.c = b.c; a.W = b.W;
        a.table.alias(b.table); a.table29.alias(b.table29); a.table29s.alias(b.table29s); a.h.alias(b.h);
        // the host-side Lagrange basis is derived from the SRS: the view keeps its copy (or one it computed itself) until the parent's SRS or domain changes
        if (a.srs_gen != b.srs_gen || a.lagrange_log2 != b.lagrange_log2 || (a.lagrange_host.empty() && !b.lagrange_host.empty())) { a.lagrange_host = b.lagrange_host; a.lagrange_log2 = b.lagrange_log2; a.srs_gen = b.srs_gen; }
        a.lagrange_table.alias(b.lagrange_table); a.lagrange_table_n = b.lagrange_table_n; a.lagrange_table_log2 = b.lagrange_table_log2;
        a.lagrange_digits.alias(b.lagrange_digits); a.lagrange_digits29.alias(b.lagrange_digits29); a.lagrange_digits_n = b.lagrange_digits_n;
    }
};

struct MsmWorkspace {
    DevBuf scalars, points, points29 /* the 2^261-domain twin of a variable-base MSM's points (api_msm.hip mb_msm_variable) */, ekey, eval, eoff, count, start, task_start, rem_pos, rem_bucket, info, sorted, partial, heavy, order, redo, ghist, stage, buckets, red_r, red_ws, red2_r, red2_w, set_total, out_words, out_xyzz, buckets29, seg_bad;
    DevBuf tail_rows, tail_tickets;    // the fused tail (msm.cuh msm_tail_kernel): a pair of XYZZ records per row of 128 buckets, a ticket word per bucket set and per problem
};

// HIP-event stage timing on the context stream (off by default; bench.py turns it on for the timed region)
enum ProfStage : int { PS_DIGITS = 0, PS_SCAN, PS_SCATTER, PS_ACCUMULATE, PS_BUCKET_SUM, PS_REDUCE_A, PS_REDUCE_BC, PS_FINISH,
                       PS_BPOLY_TABLES, PS_BPOLY_FOLD, PS_BPOLY_FINISH, PS_STATE_HASH, PS_IPA_TRANSCRIPT, PS_KIMCHI, PS_PICKLES,
                       PS_STATE_HASH1 /* the single-lane launches inside PS_STATE_HASH */, PS_COUNT };
struct ProfState {
    int mask = 0;                                   // bit per stage; 0 = off
    struct Rec { hipEvent_t a, b; int stage; };
    std::vector<Rec> recs; size_t used = 0;
};

// A pipeline lane: one HIP stream + every scratch buffer a call needs.  Independent `_dev` calls are
// issued round-robin over the lanes so that the low-occupancy tail of one MSM overlaps the wide phases of
// the next (SRS tables, field constants and Poseidon constants are shared, read-only).
struct Lane {
    hipStream_t stream = nullptr;
    hipStream_t aux = nullptr;               // second stream for work that can run beside the lane's main stream (IPA to_group)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_leg = nullptr;   // ev_leg: fork / join of the Proof-of-State job's legs
    hipEvent_t ev_done = nullptr; bool on_roles = false;                 // a pipeline lane under the role plan (state_job.hip JobRoute): recorded behind the verdict kernel of the lane's last job; on_roles: that job ran on the role streams
    MsmWorkspace ws;
    DevBuf tmp_a, tmp_b, tmp_c, tmp_d;       // staging for the host-buffer entry points
    PinnedBuf host_stage;                    // pinned host side of the big H2D blobs (synchronous entry points only)
    DevBuf bp_ltab, bp_htab, bp_partial, bp_ldig, bp_hdig, bp_colsum;
    DevBuf bp_seg_ids; PinnedBuf bp_seg_stage;   // mina_b_poly_fold_segments_dev: the ids of its matrix-core segments and their pinned host side (written only behind that call's wait for the lane)
    DevBuf ipa_chals, ipa_folded, ipa_xyzz_a, ipa_xyzz_b, ipa_points, ipa_scalars, ipa_sigma, ipa_in_a, ipa_in_b, ipa_in_c, ipa_verdict, ipa_xfer, ipa_shared, ipa_shared_off, acc_rho_scaled /* exchange variant: the caller's acc_rho times the shard's own CSPRNG scalar */;
    DevBuf st_ok, st_hashes, st_pub_xyzz, st_pubcomm, st_flags, st_in, st_verdicts;   // Proof-of-State job (api_state.hip)
    DevBuf st_masks;                         // its masks form (api_state.hip state_job_checks): chain | statement | opening culprits | accumulator culprits | front | deny | passed | ran, batch u32 each
    DevBuf dd_rep, dd_uniq, dd_table, dd_counts;  // its deduplicated state leg (state_dedup.cuh): 4 B x n each, the table 16 B x the power of two >= 2 n, counters + one word per 1024 states
    DevBuf pk_off, pk_len, pk_status, pk_info, pk_fmt;   // the packed-on-device front end (state_pack.cuh; api_pack.hip): 8 B + 4 B + 1 B per state, two info structs + 1 B per proof
    DevBuf ac_ws, ac_in;                     // the device path of a Proof-of-Account job (account_pack.cuh; api_account_dev.hip): its workspace (AccountWs), the uploaded bytes + verdict words of a boundary call
    DevBuf gs_tab, gs_folded, gs_xa, gs_xb, gs_chals, gs_points, gs_bad, gs_flags;   // the grouped culprit search (api_ipa.hip mb_*_check_parts): segment tables, one folded vector and two sums per part, the accumulator leg's challenges / checked points / per-proof malformed words, one flag per part
    DevBuf kc_state, kc_pos, kc_cip, kc_pts, kc_v, kc_u, kc_comms, kc_xfer, kc_pch, pk_xe, pk_pub, pk_ok;                  // kimchi to_batch output rows (api_kimchi.hip)
};
// ---- how the legs of pipelined device-resident jobs are laid over streams (state_job.hip dev_fork_lanes).  Streams only run side by side on separate hardware
// queues, a stream's event wait is a barrier in the queue it shares, and the process has GPU_MAX_HW_QUEUES of them, one of which serves the caller's null stream:
// `budget` = the streams the context may keep busy.  Pure: no HIP call.
//   plan A (roles = false): every pipeline lane forks its job's three legs onto helper streams of its own, 4 streams per lane -- when they fit the budget, and
//     always for a lone job (one lane, or a pinned context).
//   plan B (roles = true): the jobs of all lanes flow FIFO through shared ROLE streams: H (every job's state hashes and chain check) and `sets` pairs W1[j] / W2[j]
//     for the jobs of the lanes with lane % sets == j (W1: Pickles statement -> public-input commitment -> kimchi to_batch; W2: accumulator check, opening check,
//     verdict kernel): 1 + 2 sets streams, sets = clamp((budget - 1) / 2, 1, lanes).  A budget below 3 cannot hold the three roles apart: W1 and W2 of the one
//     set share a stream at 2, and H joins them at 1 (or less), so that the plan never keeps more than max(budget, 1) streams busy.
//     A budget that holds one stream more than those 1 + 2 sets (4, 6, 8 ..., and every budget the lane count clamps the sets under) gives the hashes a SECOND
//     carrier, H1: the jobs of the odd lanes hash on it, so that the hash launches of two consecutive jobs are resident together and the workgroups of the later
//     one fill the wave slots the earlier one frees as it drains (a whole leg is 4.25 workgroups per CU: alone on the chip its last fifth runs on a quarter of the
//     CUs; profiles/r10_hash_carriers.md).  Once H no longer sets the pace the chain streams do: each is ONE FIFO stream that serves every job of its set, and W2
//     carries half as much again as W1 (per job beside resident hashes: W1 36 ms, W2 55 ms, 18 ms of it the opening check).  With two carriers the opening check of
//     every other job of a set therefore follows its kimchi stage on W1 (check_on_w1; W2 keeps the accumulator check, the joins and the verdict kernel of every
//     job): all of them on W1 made W1 the slow stream instead (measured; same note).  sets, streams, w1 and w2 are what they are without H1.
static constexpr int MB_DEV_FORK_MAX = 8;                  // pipelines of up to this many lanes fork the legs of a device-resident job (mina_verify_tuning.dev_fork)
static constexpr int MB_ROLE_STREAMS = 2 + 2 * MB_DEV_FORK_MAX;      // H + a W1 / W2 pair per lane at the most + H1 (StreamPlan)
static constexpr int MB_ROLE_H1 = MB_ROLE_STREAMS - 1;     // the second carrier's place among the role streams: behind every pair, whatever the budget
struct StreamPlan {
    bool roles = false; int sets = 0, streams = 0;            // streams: the role streams of plan B less H1 (index 0 = H); 0 under plan A
    int carriers = 0;                                         // streams that carry state hashes under plan B: 1 (H) or 2 (H and H1); 0 under plan A
    int w1(int lane) const { return streams >= 3 ? 1 + 2 * (lane % sets) : streams - 1; }
    int w2(int lane) const { return streams >= 3 ? 2 + 2 * (lane % sets) : streams - 1; }
    int h(int lane) const { return carriers >= 2 && (lane % carriers) ? MB_ROLE_H1 : 0; }       // consecutive lanes alternate
    int busy() const { return streams + (carriers >= 2 ? 1 : 0); }                              // streams the plan keeps busy
    bool check_on_w1(int lane) const { return carriers >= 2 && ((lane / sets) & 1) == 0; }     // every other lane of a set
};
static inline StreamPlan stream_plan(int lanes_in_flight, int budget) {
    StreamPlan p;
    if (lanes_in_flight <= 1 || 4 * lanes_in_flight <= budget) return p;
    p.roles = true;
    p.sets = std::min(std::max((budget - 1) / 2, 1), lanes_in_flight);
    p.streams = std::min(1 + 2 * p.sets, std::max(budget, 1));
    p.carriers = (p.streams >= 3 && budget > p.streams) ? 2 : 1;
    return p;
}
// The plan of a context that forces no budget, from the environment's (env_stream_budget: the queues less the one the caller's null stream runs on).  Plan A is
// decided on that budget.  The role plan may take the last queue as well where that buys the second carrier: under plan B the library queues nothing on the
// caller's stream or on the lanes' own, so the queue held back for the caller carries nothing while jobs flow, and the one role stream that ends up beside the
// caller's stream loses nothing to it unless the caller queues work of its own there -- which then waits behind that stream's kernels, as it did behind W1's
// before (the runtime dealt W1 the caller's queue and left the fourth empty: profiles/r08_role_streams.md, r10_hash_carriers.md).  Taken with four lanes or more
// in flight only: that is where the two-carrier plan was timed against the plain one (4 lanes; more lanes queue behind the same four streams), and with 2 or 3
// lanes, which nobody timed, a context that forces no budget keeps the plan it had.  mina_ctx_set_stream_budget(4) gives two carriers at any lane count.
static constexpr int MB_ENV_H1_MIN_LANES = 4;
static inline StreamPlan stream_plan_env(int lanes_in_flight, int env_budget) {
    const StreamPlan p = stream_plan(lanes_in_flight, env_budget);
    if (!p.roles || p.carriers >= 2 || lanes_in_flight < MB_ENV_H1_MIN_LANES) return p;
    const StreamPlan q = stream_plan(lanes_in_flight, env_budget + 1);
    return (q.roles && q.carriers >= 2 && q.sets == p.sets) ? q : p;
}
// The piece, in waves, of a state-hash leg of `leg_waves` waves under plan B with two carriers (0: one launch).  Two carriers hold the pieces of two jobs resident
// together, so pieces pay again (on a lone H they only idle wave slots between launches): 4 lanes, the leg of 4352 single-lane waves, one box -- whole 286 k
// proofs/s, 3072: 306 - 308 k, 1792 / 1664 / 1536 / 1451: 311 / 311 / 312 - 313 / 310 k, beside the parent's 292 - 297 k; but 2048, 1408, 1280 and 1024, which
// leave a last piece of 256, 128, 512 and 256 waves: 298 / 284 / 285 / 293 k -- a thin piece holds its carrier for as long as a full one.  Hence EQUAL pieces,
// as many as a target of 6144 / lanes waves asks for (half plan A's 12 288 / lanes: 1536 at 4 lanes), and half that in the 3-lane form, whose waves hold a third
// of the states (by plan A's ratio; not measured).  profiles/r10_hash_carriers.md.  Pure.
static inline uint32_t role_piece_waves(size_t leg_waves, int lanes_in_flight, bool one_lane) {
    const size_t target = (one_lane ? 6144u : 3072u) / (size_t)std::max(lanes_in_flight, 1);
    if (target == 0 || leg_waves <= target) return 0;
    const size_t n = (leg_waves + target - 1) / target;
    return (uint32_t)((leg_waves + n - 1) / n);
}
// GPU_MAX_HW_QUEUES as the process has it (the library's load-time constructor sets a default where it is unset: api_core.hip), 1 .. 32, less the caller's null stream
static inline int env_stream_budget() {
    const char *e = getenv("GPU_MAX_HW_QUEUES");
    const long q = e ? strtol(e, nullptr, 10) : 4;
    return (int)std::min(std::max(q, 1L), 32L) - 1;
}
static constexpr int MB_PIPE_LANES = 32;                   // lanes a caller may pipeline over (mina_ctx_set_pipeline) = the fan-out of the culprit search
static constexpr int MB_DEV_HELPER0 = MB_PIPE_LANES + 3 * 16;   // helper lanes of pipeline lane i: MB_DEV_HELPER0 + 3 i .. (wrap-proof chain / accumulator / state hashes)
// The helper lanes of the forked device-resident jobs own NO stream: their `stream` is an alias of one of the context's fork streams (mina_ctx::fork_own, plan A)
// or role streams (mina_ctx::role, plan B), which the context creates and destroys once.
static constexpr int MB_MAX_LANES = MB_DEV_HELPER0 + 3 * MB_DEV_FORK_MAX;  // pipeline lanes + the helper lanes of the boundary's 16 slots (api_verify.hip: legs of slot s on lanes 32 + 3 s ..) + those of the forked device-resident jobs
enum : int { MB_SALT_PSTATE_BODY = 0, MB_SALT_PSTATE, MB_SALT_ACCOUNT, MB_SALT_ZKAPP_ACCOUNT, MB_SALT_ZKAPP_URI, MB_SALT_SIDE_LOADED_VK, MB_N_PREFIX_SALTS };

// An INDEX SET: everything that belongs to one installed (wrap index, step index) pair.  A context holds two, numbered 0 and 1 -- the boundary keeps one per Mina
// network (api_verify.hip, net_route.h) -- and one of them is SELECTED: its fields are the ones below, inherited by Installed under their old names, so that every
// installer, getter and launch site reads the selected set without knowing of the other, which is parked beside them (Installed::parked).
struct IndexSet {
    DevBuf kimchi_index, kimchi_tokens, kimchi_literals; bool have_kimchi = false; uint32_t kimchi_log2 = 0; uint8_t kimchi_digest[32] = {0};   // installed wrap verifier index
    uint8_t kimchi_comms_host[28 * 64] = {0};   // its commitments as installed: sigma 7, coefficients 15, selectors 6 (messages_for_next_step_proof hashes them)
    DevBuf pickles_index, pickles_tokens, pickles_literals; bool have_pickles_dev = false, pickles_ms_valid = false;   // installed step index (api_pickles.hip); ms = the Tick sponge after the wrap index commitments
    void *step_host = nullptr; void (*step_host_free)(void *) = nullptr;   // host half of the installed step index (api_pickles.hip), owned by the context
    inline void swap_set(IndexSet &o) {          // handles and host fields change places: no HIP call, no allocation; launches already queued keep the pointers they captured
        kimchi_index.swap(o.kimchi_index); kimchi_tokens.swap(o.kimchi_tokens); kimchi_literals.swap(o.kimchi_literals);
        std::swap(have_kimchi, o.have_kimchi); std::swap(kimchi_log2, o.kimchi_log2); std::swap(kimchi_digest, o.kimchi_digest); std::swap(kimchi_comms_host, o.kimchi_comms_host);
        pickles_index.swap(o.pickles_index); pickles_tokens.swap(o.pickles_tokens); pickles_literals.swap(o.pickles_literals);
        std::swap(have_pickles_dev, o.have_pickles_dev); std::swap(pickles_ms_valid, o.pickles_ms_valid);
        std::swap(step_host, o.step_host); std::swap(step_host_free, o.step_host_free);
    }
    inline void borrow_set(const IndexSet &p) {  // a view context's: the buffers aliased, the host half borrowed
        IndexSet *const v = this;
        v->kimchi_index.alias(p.kimchi_index); v->kimchi_tokens.alias(p.kimchi_tokens); v->kimchi_literals.alias(p.kimchi_literals);
        v->have_kimchi = p.have_kimchi; v->kimchi_log2 = p.kimchi_log2; memcpy(v->kimchi_digest, p.kimchi_digest, sizeof v->kimchi_digest); memcpy(v->kimchi_comms_host, p.kimchi_comms_host, sizeof v->kimchi_comms_host);
        v->pickles_index.alias(p.pickles_index); v->pickles_tokens.alias(p.pickles_tokens); v->pickles_literals.alias(p.pickles_literals);
        v->have_pickles_dev = p.have_pickles_dev; v->pickles_ms_valid = p.pickles_ms_valid;
        // borrowed: the parent frees it.  A host half the view had built for itself (step_of(view) before the parent had one) is freed first (it leaked)
        if (v->step_host && v->step_host_free && v->step_host != p.step_host) v->step_host_free(v->step_host);
        v->step_host = p.step_host; v->step_host_free = nullptr;
    }
    inline void free_step_host() { if (step_host && step_host_free) step_host_free(step_host); step_host = nullptr; step_host_free = nullptr; }
    inline void clear() {                        // back to "nothing installed": the buffers freed; the hazard and the locking are an install's
        kimchi_index.release(); kimchi_tokens.release(); kimchi_literals.release(); pickles_index.release(); pickles_tokens.release(); pickles_literals.release();
        have_kimchi = false; kimchi_log2 = 0; memset(kimchi_digest, 0, sizeof kimchi_digest); memset(kimchi_comms_host, 0, sizeof kimchi_comms_host);
        have_pickles_dev = false; pickles_ms_valid = false;
        free_step_host();
    }
};

// Everything INSTALLED on a context: what a view context borrows from its parent -- borrow_from, directly under the fields it must stay in step with.
// The two index sets are per pair; everything else -- field constants, both SRS and their Lagrange tables, Poseidon tables, salts -- is shared by both.
struct Installed : IndexSet {
    FieldK fk[2];
    SrsState srs[2];
    DevBuf pparams[2]; bool have_pparams[2] = {false, false};
    bool pparams_surrogate[2] = {false, false};                  // the installed Poseidon tables are the library's UNPINNED surrogate set
    bool pparams_rows1[2] = {false, false};                      // the installed tables have the single-lane form's normalised rows (sponge.cuh PoseidonRows1: no zero on the MDS diagonal)
    DevBuf merkle_salts[2]; uint32_t merkle_depth[2] = {0, 0};   // salted initial states of the Merkle hash per height
    IndexSet parked; uint32_t index_set = 0;                     // the index set that is NOT selected, and the number (0 | 1) of the one that is (mina_ctx_select_index_set)
    DevBuf state_salts; bool have_state_salts = false;           // salted initial states of the named hash prefixes (Fp): MB_SALT_*
    inline IndexSet &set_at(uint32_t k) { return k == index_set ? static_cast<IndexSet &>(*this) : parked; }
    inline const IndexSet &set_at(uint32_t k) const { return k == index_set ? static_cast<const IndexSet &>(*this) : parked; }
    // Host bookkeeping only: no HIP call, no allocation, no synchronisation.  The caller holds whatever serialises installs and jobs on the context.
    inline void select_index_set(uint32_t k) { if (k != index_set) { swap_set(parked); index_set = k; } }
    // what the Poseidon tables of Fp went into, in BOTH sets: the Tick sponge after the wrap index commitments (mina_poseidon_set_params)
    inline void invalidate_table_derived() { pickles_ms_valid = false; parked.pickles_ms_valid = false; }
    inline void borrow_from(const Installed &p) {                // set k of the view borrows set k of the parent; the view keeps its own selection
        Installed *const v = this;
        for (int i = 0; i < 2; ++i) {
            v->fk[i] = p.fk[i];
            v->srs[i].borrow_from(p.srs[i]);
            v->pparams[i].alias(p.pparams[i]); v->have_pparams[i] = p.have_pparams[i]; v->pparams_surrogate[i] = p.pparams_surrogate[i]; v->pparams_rows1[i] = p.pparams_rows1[i];
            v->merkle_salts[i].alias(p.merkle_salts[i]); v->merkle_depth[i] = p.merkle_depth[i];
        }
        for (uint32_t k = 0; k < 2; ++k) v->set_at(k).borrow_set(p.set_at(k));
        v->state_salts.alias(p.state_salts); v->have_state_salts = p.have_state_salts;
    }
};

struct mina_ctx : Installed {
    int device = 0;
    ProfState prof;
    Lane lanes[MB_MAX_LANES];
    int nlanes = 1;
    unsigned rr = 0;                 // round-robin cursor of the `_dev` entry points
    int pinned = -1;                 // >= 0: every `_dev` entry point runs on this lane (mina_ctx_pin_lane): a caller that queues its own work on that lane's stream needs no host synchronisation
    Lane *L = nullptr;               // lane the current call runs on
    Lane *ipa_rows = nullptr; uint32_t ipa_rows_batch = 0, ipa_rows_k = 0, ipa_rows_per = 0, ipa_rows_nshared = 0; int ipa_rows_curve = -1;   // lane holding the prepared rows of the last folded opening check (mb_ipa_recheck_rows)
    bool is_view = false;            // a view of another context (mb_ctx_create_view: the culprit search's): creates no stream beyond its lane 0 -- its lanes 1 .. 3 borrow the failed chunk's, and the opening check's side stream is off
    bool state_dedup = false;        // the protocol-state leg of a job hashes each distinct record once (mina_ctx_set_state_dedup; api_state.hip pstate_hash_dedup_dev)
    DevBuf dedup_totals; uint64_t dedup_states = 0;   // mina_ctx_state_dedup_stats: {distinct, collisions} summed on the device by the legs' scan kernels, the states counted as they are queued
    // mina_state_frontend_dev without the argument checks, queued on the CURRENT lane (api_pack.hip mb_state_frontend_on_lane).  Filled by mina_ctx_create; the
    // boundary reaches the device front end through it (MINA_VERIFY_PACK_ON_DEVICE), and a context without it -- the stand-in contexts of the ThreadSanitizer tier,
    // which link no kernel -- keeps the host path.
    int (*state_frontend)(mina_ctx *c, size_t batch, const void *d_blob, size_t blob_len, const void *d_begin, const void *d_end, const void *d_expected_hashes,
                          const void *d_ledger_hashes, const void *d_and, void *d_records, void *d_nfields, void *d_precheck, void *d_masks) = nullptr;
    // Proof-of-Account on the device (api_account_dev.hip).  acct_defaults: the hashes of the empty URI, the dummy verification key and the default zkApp record under
    // the installed Fp tables (3 x 8 canonical words + their three records), computed on first use, dropped when the tables change.  account_on_device: the device
    // twin of mb_verify_account_on (same arguments), filled by mina_ctx_create; the boundary reaches it through the pointer (MINA_VERIFY_ACCOUNT_ON_DEVICE), and a
    // context without it keeps the host path.
    DevBuf acct_defaults; bool have_acct_defaults = false;
    int (*account_on_device)(mina_ctx *c, size_t n, const uint8_t *const *proofs, const size_t *proof_lens, const uint8_t *const *pubs, const size_t *pub_lens,
                             uint32_t *passed, uint32_t *ran, Lane *lane, std::mutex *enq_mu) = nullptr;
    // The grouped culprit search of a failed job (mina_ctx_set_search_groups; api_state.hip): 0 = the fan search.  The counters of mina_ctx_search_stats follow from
    // (batch, groups, culprits) alone: searches = legs searched in groups, rounds = levels, parts = segments checked.
    uint32_t search_groups = 0; uint64_t gs_searches = 0, gs_rounds = 0, gs_parts = 0;
    // The segmented b_poly fold (api_sponge.hip run_bpoly_fold_segments): segments of seg_fold_mfma_min proofs or more, and fewer than 2^17, are folded on the matrix
    // cores (mina_ctx_set_seg_fold_mfma_min; 0 = never; 256 = the single fold's rule).  mina_ctx_seg_fold_stats: segments folded by either kind of kernel and
    // matrix-core passes, counted as they are queued by the context that ran the fold.
    uint32_t seg_fold_mfma_min = 256; uint64_t sf_mfma_segments = 0, sf_valu_segments = 0, sf_mfma_passes = 0;
    // The fused MSM tail (mina_ctx_set_msm_fused_tail; api_msm.hip MsmPlan::fused_tail): task-form MSMs run bucket sums, reduction and finish as ONE launch.
    // mina_ctx_msm_tail_stats: MSMs queued with either tail, counted by the context that queued them.
    bool msm_fused_tail = false; uint64_t mt_fused_runs = 0, mt_staged_runs = 0;
    // The fast inverse (mina_ctx_set_fast_inverse): the one inversion at the end of an MSM -- msm_finish_kernel's, or the fused tail's -- is the divstep iteration of
    // fe_modinv.cuh instead of the power p - 2; the same bytes.  mina_ctx_inverse_stats: MSM finishes queued with either form, counted by the context that queued them
    // (an MSM whose reduction kernel hands out the XYZZ result itself has no finish and counts as neither).
    bool fast_inverse = false; uint64_t inv_gcd_finishes = 0, inv_fermat_finishes = 0;
    // The chain inverse (mina_ctx_set_chain_inverse): the single-lane inversions of the wrap-proof chain's scalar stages and of the Lagrange set-up -- ft_eval0 (both
    // sides), the public polynomial, the ft commitment, the public-input commitment finishes, the Lagrange basis and its digit table, mina_points_sum_dev -- run the
    // `_gcd` twin of their kernel (fe_modinv.cuh) instead of the power p - 2; the same bytes.  Independent of fast_inverse, which stays the MSM finish alone.
    // mina_ctx_chain_inverse_stats: launches of those kernels by form, counted by the context that queued them (gcd_launch() below, once per launch).
    bool chain_inverse = false; uint64_t chain_gcd_launches = 0, chain_fermat_launches = 0;
    bool gcd_launch() { ++(chain_inverse ? chain_gcd_launches : chain_fermat_launches); return chain_inverse; }
    uint64_t search_streams_made = 0;  // streams any culprit search of this context has created (the fan search, for the lanes it lacks): mina_ctx_lane_streams
    // mina_state_job_batch without its upload: per-proof verdicts (host bytes) of a job whose inputs are in HBM, on lane 0, waited for (api_state.hip
    // mb_state_job_each_host).  Filled by mina_ctx_create; the boundary hands a failed chunk's device staging to it under MINA_VERIFY_GROUPED_SEARCH, and a context
    // without it -- the stand-in contexts of the ThreadSanitizer tier -- keeps the host-buffer path.
    int (*state_job_each)(mina_ctx *c, const mina_state_jobs *dev_jobs, uint8_t *verdicts) = nullptr;
    // MIXED jobs (StateJobPlan::d_net: proof b against index set d_net[b]; include/mina_verify.h "MIXED jobs").  The two stages of the wrap-proof leg that read index
    // data, in their `_net` forms (api_pickles.hip mb_pickles_statements_net_dev, api_kimchi.hip mb_kimchi_to_batch_net_dev).  Filled by mina_ctx_create; state_job.hip
    // reaches them through the pointers, and a context without them -- the stand-in contexts of the trace and ThreadSanitizer tiers, which link no kernel -- cannot
    // queue a mixed job (MINA_ERR_STATE).
    // mixed_jobs, mixed_totals (mina_ctx_mixed_job_stats): jobs queued with d_net, counted as they are queued; their proofs by set, two 64-bit words summed on the
    // device by the kimchi stage's counting launch (the bytes are in HBM), allocated and zeroed by the first mixed job (mb_ctx_mixed_totals).
    int (*pickles_statements_net)(mina_ctx *c, size_t batch, const mina_pickles_statements *s, uint32_t *d_pub, uint32_t *d_ok, const uint8_t *d_net) = nullptr;
    int (*kimchi_to_batch_net)(mina_ctx *c, size_t batch, uint32_t n_prev, uint32_t npub, const mb::KimchiIn &in, const mb::KimchiOut &out, uint32_t *d_bad, const uint8_t *d_net,
                               const void *pf_digest, uint32_t pf_stride, void *d_count) = nullptr;
    // state_job_each for a mixed job (api_state.hip mb_state_job_each_net_host): per-proof verdict bytes of a job in HBM with its bytes d_net, on lane 0, waited for.
    // The boundary's fallback runs it over a failed mixed chunk's device staging; a context without it never gets a mixed pass (api_verify.hip ShapePass::run).
    int (*state_job_each_net)(mina_ctx *c, const mina_state_jobs *dev_jobs, const uint8_t *d_net, uint8_t *verdicts) = nullptr;
    int (*mixed_sets_check)(mina_ctx *c) = nullptr;      // mb_mixed_sets_check: the preconditions of a mixed launch, MINA_ERR_STATE where they do not hold
    uint64_t mixed_jobs = 0; DevBuf mixed_totals;
    // The masks form of the job (api_state.hip mb_state_job_checks_host): `passed` / `ran` words (host) of a job whose inputs are in HBM, on lane 0, waited for.
    // front: the front end's d_masks in HBM (d_front), or host words to upload (front), or neither; deny: host words or null.  Filled by mina_ctx_create; the boundary's
    // mina_verify_state_checks_batch reaches the body through it, and a context without it -- the stand-in contexts of the ThreadSanitizer tier -- answers proof by
    // proof through the single-proof form.  checks_jobs / checks_proofs (mina_ctx_checks_stats): the full job passes checks calls have queued, and the proofs in them.
    int (*state_job_checks)(mina_ctx *c, const mina_state_jobs *dev_jobs, const uint32_t *d_front, const uint32_t *front, const uint32_t *deny, uint32_t *passed, uint32_t *ran) = nullptr;
    uint64_t checks_jobs = 0, checks_proofs = 0;
    uint32_t dev_fork_made = 0;      // the dev_fork value the helper lanes' streams were created under (streams keep their mask / priority for life)
    // The streams behind the helper lanes of the forked jobs (StreamPlan), created on first use, destroyed once by mina_ctx_destroy: plan A's, three per pipeline
    // lane, and plan B's role streams.  stream_budget: forced by mina_ctx_set_stream_budget (> 0), else the environment's, read when the first job forks (-1: not yet).
    hipStream_t fork_own[3 * MB_DEV_FORK_MAX] = {}; hipStream_t role[MB_ROLE_STREAMS] = {};
    int stream_budget = 0, stream_budget_env = -1;
    StreamPlan last_plan;            // the plan the last forked device-resident job was queued under (mina_ctx_stream_plan_stats); all zero before the first
    void use_lane0() { L = &lanes[0]; }
    void next_lane() { L = pinned >= 0 ? &lanes[pinned] : &lanes[rr++ % (unsigned)nlanes]; }
};
static inline void mb_ctx_refresh_view(mina_ctx *view, mina_ctx *parent) { view->borrow_from(*parent); view->msm_fused_tail = parent->msm_fused_tail; view->fast_inverse = parent->fast_inverse; view->chain_inverse = parent->chain_inverse; }

// waits for everything the `_dev` entry points have queued: the pipeline lanes and, for jobs that ran under plan B, the role streams
static inline hipError_t mb_ctx_wait_all(mina_ctx *c) {
    for (int i = 0; i < c->nlanes; ++i) if (c->lanes[i].stream) { hipError_t e = hipStreamSynchronize(c->lanes[i].stream); if (e != hipSuccess) return e; }
    for (hipStream_t s : c->role) if (s) { hipError_t e = hipStreamSynchronize(s); if (e != hipSuccess) return e; }
    return hipSuccess;
}

// mina_ctx_set_state_dedup without the argument checks (the boundary switches its contexts under their lock: api_verify.hip finish()).  The statistics start
// again whenever the mode goes from off to on; that waits for the pipeline lanes.
static inline int mb_ctx_state_dedup(mina_ctx *c, bool on) {
    if (on && !c->state_dedup) {
        if (mb_ctx_wait_all(c) != hipSuccess) return MINA_ERR_HIP;
        int rc = c->dedup_totals.ensure(16);
        if (rc) return rc;
        if (hipMemsetAsync(c->dedup_totals.p, 0, 16, c->lanes[0].stream) != hipSuccess || hipStreamSynchronize(c->lanes[0].stream) != hipSuccess) return MINA_ERR_HIP;
        c->dedup_states = 0;
    }
    c->state_dedup = on;
    return MINA_OK;
}

// the device words of mina_ctx_mixed_job_stats, allocated and zeroed before the context's first mixed job (that once, it waits for lane 0)
static inline int mb_ctx_mixed_totals(mina_ctx *c) {
    if (c->mixed_totals.p) return MINA_OK;
    int rc = c->mixed_totals.ensure(16);
    if (rc) return rc;
    if (hipMemsetAsync(c->mixed_totals.p, 0, 16, c->lanes[0].stream) != hipSuccess || hipStreamSynchronize(c->lanes[0].stream) != hipSuccess) return MINA_ERR_HIP;
    return MINA_OK;
}

// lane-cooperative Poseidon: batches of at most this many sponges use 8 lanes each (shortest dependency chain, 2.6x the issue
// slots), larger ones the wave-packed 3-lane form (21 sponges per wave); both run their rounds on the 29-bit limbs (fp29.cuh).
// The per-proof transcripts of a job (kimchi, Pickles statement, opening) switch at 1024 proofs per call instead (transcript_lanes:
// measured with 16 calls in flight).
static constexpr size_t COOP8_MAX_GROUPS = 8192;   // (the default of mina_verify_tuning.coop8_max)
// `groups` sponges per call, `nlanes` calls in flight: the choice looks at the work in flight (256 proofs per call on 16 lanes are 69 k state
// hashes at once -- the 8-lane form then spends 2.1x the issue slots of a saturated chip: 480 proofs per call 66 -> 75 k/s).
// mina_verify_tuning.coop8_max overrides the limit, .coop8_per_call = 1 ignores the lanes.
static inline bool use_coop8(const mina_ctx *c, size_t groups) {
    const mina_verify_tuning t = mb_tune();
    return groups * (size_t)((c && !t.coop8_per_call) ? c->nlanes : 1) <= (size_t)t.coop8_max;
}

// One proof or a handful in flight (the reference's call pattern): 16 lanes per sponge -- the shortest dependent chain, at 5.3x the issue
// slots of the 3-lane form (poseidon_permute_hex).  `proofs` per call x lanes in flight, up to 64 (one proof 25.5 -> 23.1 ms, 16 proofs
// 22.9 -> 21.2 ms; at 256 the 8-lane form is as fast); mina_verify_tuning.coop16_max overrides (0 disables).
static inline bool use_coop16(const mina_ctx *c, size_t proofs) {
    return proofs * (size_t)(c ? c->nlanes : 1) <= (size_t)mb_tune().coop16_max;
}

// The per-proof transcripts (statement, kimchi, opening): 8 lanes per sponge while the proofs in flight (per call x lanes) leave the chip
// latency-bound (<= 1024 per call and <= 2048 in flight: with 16 lanes 1024 per call ran 123 k/s in the 8-lane form, 138 k/s in the 3-lane
// form; 512: 83 / 91 k; 256: 54 / 58 k), the wave-packed 3-lane form beyond.  mina_verify_tuning.transcript_coop8_max overrides (proofs in flight).
static inline bool use_coop8_transcripts(const mina_ctx *c, size_t batch, size_t per_call_limit) {
    const size_t lim = (size_t)mb_tune().transcript_coop8_max;
    const size_t in_flight = batch * (size_t)(c ? c->nlanes : 1);
    return lim ? in_flight <= lim : ((batch <= per_call_limit && in_flight <= 2048) || in_flight <= 2560);   // a call alone on the GPU: 1536 proofs 29.2 -> 26.8 ms, 2048: 30.2 -> 28.4, 3072: flat, 4096: +3 ms
}

// The protocol-state hashes of a leg of `leg_states` states run ONE lane per state (api_state.hip pstate_hash1_kernel: the fewest instructions per hash, the
// longest chain per wave) when the installed tables have the normalised rows, several jobs are in flight and they hold HASH1_MIN_STATES states or more between
// them (64 per wave: 65 536 are one wave per SIMD of the chip).  A lone job keeps the 3-lane form: its hashes run beside the job's own chain, as one launch
// behind the LDS reservation tuned for that form (HashLaunch::lds_bytes), and a lone 4096-proof call would be one single-lane wave per SIMD.
static constexpr size_t HASH1_MIN_STATES = 65536;
static inline int hash_jobs_in_flight(const mina_ctx *c) { return c->pinned >= 0 ? 1 : c->nlanes; }      // a pinned context runs one job at a time
static inline bool hash_one_lane(const mina_ctx *c, size_t leg_states) {
    const int jobs = hash_jobs_in_flight(c);
    return c->pparams_rows1[FIELD_FP] && jobs >= 2 && leg_states * (size_t)jobs >= HASH1_MIN_STATES;
}
// states per launch piece of such a leg (0: one launch): `piece_waves` waves of the form that runs -- 64 states each in the single-lane form, 21 in the 3-lane form
static inline size_t hash_piece_states(const mina_ctx *c, size_t leg_states, uint32_t piece_waves) { return (size_t)piece_waves * (hash_one_lane(c, leg_states) ? 64u : 21u); }

// ---- the lane form of each kind of sponge work: lanes per sponge, launched through with_lanes below.  Each site has exactly one of these rules.
// Salted hashes (the account hashes; the protocol-state hashes behind their single-lane test): `proofs` decides the 16-lane form, `sponges` the 8-lane one.
static inline int hash_lanes(const mina_ctx *c, size_t proofs, size_t sponges) { return use_coop16(c, proofs) ? 16 : (use_coop8(c, sponges) ? 8 : 3); }
// `n` protocol-state hashes of a leg of `leg_states` (api_state.hip pstate_hash_dev); the 16-lane test counts the proofs those `n` states make up
static inline int pstate_hash_lanes(const mina_ctx *c, size_t n, size_t leg_states) {
    return hash_one_lane(c, leg_states) ? 1 : hash_lanes(c, (n + MINA_STATES_PER_PROOF - 1) / MINA_STATES_PER_PROOF, n);
}
// The per-proof transcripts: the Pickles statement passes 1024 proofs per call, kimchi mina_verify_tuning.kimchi_coop8_max and the opening check .ipa_coop8_max
// (both 1024 by default).  Kimchi, measured on bench.py --kimchi with 8192 proofs per step: 16 x 512 ran 165 k/s in the 8-lane form against 162 k/s in the 3-lane
// form, 4 x 2048 137 k/s against 150 k/s.  The opening check with 16 calls of 8192 proofs in flight (bench.py), where the VALU port is what saturates: the 3-lane
// form runs 21 transcripts per wave at 3/8 of the issue slots.
static inline int transcript_lanes(const mina_ctx *c, size_t batch, size_t per_call_limit) {
    return use_coop16(c, batch) ? 16 : (use_coop8_transcripts(c, batch, per_call_limit) ? 8 : 3);
}
// mina_poseidon_hash and mina_fq_sponge_run: 8 lanes up to COOP8_MAX_GROUPS sponges per call, whatever the tuning and the calls in flight, the 3-lane form above.
// Both forms run their rounds on the 29-bit limbs (fp29.cuh), which beats one lane per sponge on the saturated 8 x 32 form at every size (19 k against 25 k
// cycles per sponge-round).
static inline int sponge_batch_lanes(size_t n) { return n <= COOP8_MAX_GROUPS ? 8 : 3; }
// the Merkle fold (api_sponge.hip mb_merkle_fold_dev): a few paths take 16 lanes each (use_coop16), the rest as sponge_batch_lanes
static inline int merkle_lanes(const mina_ctx *c, size_t paths) { return use_coop16(c, paths) ? 16 : sponge_batch_lanes(paths); }

// ---- the Proof-of-State job on the lanes of a context (state_job.hip); every pointer of `j` is a device pointer
enum : uint32_t { MB_JOB_LEGS = 1, MB_JOB_FINISH = 2, MB_JOB_ALL = 3 };
struct StateJobCarry { uint32_t *ipa_v = nullptr, *acc_v = nullptr, *kimchi_bad = nullptr; const uint32_t *stmt_ok = nullptr; };
// How the protocol-state hashes of a leg are launched (api_state.hip pstate_hash_launch).  piece_waves > 0: in pieces of this many waves of the form that runs
// (hash_piece_states).  lds_bytes > 0: dynamic LDS a state-hash workgroup reserves (3-lane or single-lane form), to cap its waves per SIMD beside the other legs of
// a forked job (mina_verify_tuning.dev_hash_lds_kb; by default only a lone job reserves, and a lone job hashes in the 3-lane form: hash_one_lane).
struct HashLaunch { uint32_t piece_waves = 0, lds_bytes = 0; };
// SURVEY.md 8e.2 (one exchange step over several GPUs): given one, the folded checks of a job do NOT run their fixed-base MSM and comparison -- they hand out
// this shard's folded scalar vector and the 17-word record of its variable-base partial sum instead (mina_state_job_fold_dev); device pointers
struct FoldExport { uint32_t *ipa_scalars = nullptr, *ipa_point = nullptr, *acc_scalars = nullptr, *acc_point = nullptr; };
// How ONE job is queued: decided by the caller (state_job.hip dev_fork_lanes, the boundary's chunks in api_verify.hip), read by mb_state_jobs_on_lane and its legs.
struct StateJobPlan {
    Lane *wrap = nullptr, *acc = nullptr, *states = nullptr;   // helper lanes of the wrap-proof / accumulator / protocol-state legs; null = the current lane
    uint32_t phase = MB_JOB_ALL; StateJobCarry *carry = nullptr;
    uint32_t *d_stmt_out = nullptr;                             // [batch] or null: the per-proof "Pickles statement well-formed" words
    size_t hashed_early = 0;                                    // states of the protocol-state leg already queued on its lane by mb_state_hashes_early
    HashLaunch hash;
    const FoldExport *fold_export = nullptr;
    const struct LegStreams *lent = nullptr;                    // device-resident jobs only (state_job.hip dev_fork_lanes): the streams lent to wrap / acc / states for this job
    // A MIXED job: proof b is checked against index set d_net[b] (batch bytes in HBM, 0 | 1) of the context instead of the selected one -- the wrap-proof leg queues the
    // `_net` forms of the Pickles statement and kimchi stages and an opening check whose only batch-shared point is h.  Null: today's launches.
    // count_mixed: false for the passes a culprit search re-queues (mina_ctx_mixed_job_stats counts a job and its proofs once).
    const uint8_t *d_net = nullptr; bool count_mixed = true;
};
// What dev_fork_lanes lends the helper lanes of a device-resident job, which own no stream: plan A's three of the pipeline lane, or plan B's roles (StreamPlan:
// wrap = W1, acc = W2, states = the lane's carrier, H or H1).  acc_first: the accumulator leg shares the hashes' lane and goes AHEAD of them
// (mina_verify_tuning.dev_acc_lane = 2).  check_on_wrap: under the role plan the opening check stays on W1 (StreamPlan::check_on_w1).
struct LegStreams { hipStream_t wrap = nullptr, acc = nullptr, states = nullptr; bool roles = false, acc_first = false, check_on_wrap = false; };
int mb_state_jobs_on_lane(mina_ctx *c, const mina_state_jobs *j, uint32_t *d_verdicts, uint32_t *d_flags, const StateJobPlan &plan = {});
int mb_verify_account_on(mina_ctx *c, size_t n, const uint8_t *const *proofs, const size_t *proof_lens, const uint8_t *const *pubs, const size_t *pub_lens,
                         uint32_t *passed, uint32_t *ran, Lane *lane, std::mutex *enq_mu);   // api_account.hip: Proof-of-Account on a lane of the caller's choice
int mb_state_frontend_on_lane(mina_ctx *c, size_t batch, const void *d_blob, size_t blob_len, const void *d_begin, const void *d_end, const void *d_expected_hashes,
                              const void *d_ledger_hashes, const void *d_and, void *d_records, void *d_nfields, void *d_precheck, void *d_masks);   // api_pack.hip
int mb_verify_account_dev_on(mina_ctx *c, size_t n, const uint8_t *const *proofs, const size_t *proof_lens, const uint8_t *const *pubs, const size_t *pub_lens,
                             uint32_t *passed, uint32_t *ran, Lane *lane, std::mutex *enq_mu);   // api_account_dev.hip: the same on the device, from the bytes as they are
int mb_state_job_each_host(mina_ctx *c, const mina_state_jobs *dev_jobs, uint8_t *verdicts);   // api_state.hip
int mb_state_job_each_net_host(mina_ctx *c, const mina_state_jobs *dev_jobs, const uint8_t *d_net, uint8_t *verdicts);   // api_state.hip: the same for a mixed job
int mb_state_job_checks_host(mina_ctx *c, const mina_state_jobs *dev_jobs, const uint32_t *d_front, const uint32_t *front, const uint32_t *deny, uint32_t *passed, uint32_t *ran);   // api_state.hip
int mb_state_hashes_early(mina_ctx *c, Lane *LS, size_t ns_total, size_t lo, size_t cnt, const uint32_t *d_records, const uint32_t *d_nfields, hipEvent_t after, HashLaunch hash);   // state_job.hip
// The device layer under state_job.hip, defined where the kernels are (api_state.hip): the argument checks of a job, the state hashes of a leg on the current
// lane (plain, or each distinct record once), and one launch function per kernel the legs launch themselves -- the same grid and block on the stream given, nothing else.
int mb_check_jobs(mina_ctx *c, const mina_state_jobs *j);
int pstate_hash_dev(mina_ctx *c, size_t n, size_t leg, HashLaunch hl, const uint32_t *d_records, const uint32_t *d_nfields, uint32_t *d_hashes, uint32_t *d_bodies);
int pstate_hash_dedup_dev(mina_ctx *c, size_t n, size_t leg, HashLaunch hl, const uint32_t *d_records, const uint32_t *d_nfields, uint32_t *d_hashes, uint32_t *d_bodies, bool count);
void mb_launch_pstate_chain_check(hipStream_t stream, uint32_t batch, const uint32_t *hashes, const uint32_t *expected, const uint32_t *records, const uint8_t *precheck, uint32_t *ok);
void mb_launch_fill_u32(hipStream_t stream, uint32_t n, uint32_t v, uint32_t *out);
void mb_launch_state_job_verdict(hipStream_t stream, uint32_t batch, const uint32_t *chain_ok, const uint32_t *ipa_v, const uint32_t *acc_v, const uint32_t *kimchi_bad,
                                 const uint32_t *stmt_ok, uint32_t *verdicts, uint32_t *flags, uint32_t *stmt_out);
void mb_launch_challenge_to_field_fq(hipStream_t stream, uint32_t n, FieldK fk, const uint32_t *chal, uint32_t *out_words);
int mb_pubcomm_dev(mina_ctx *c, size_t batch, uint32_t log2_domain, uint32_t npub, const uint32_t *d_pub, uint32_t *d_out16);      // api_state.hip
int mb_pickles_statements_dev(mina_ctx *c, size_t batch, const mina_pickles_statements *s, uint32_t *d_pub, uint32_t *d_ok);      // api_pickles.hip
void mb_pickles_kimchi_digest(mina_ctx *c, const mina_pickles_statements *s, const void **first, uint32_t *stride);
// The MIXED forms (the `_net` twins of the index-reading kernels): proof b against index set d_net[b] (0 | 1, device bytes) of the context, whichever is selected.
int mb_mixed_sets_check(mina_ctx *c);                                                                                               // api_pickles.hip: both sets fully installed, equal wrap domains; else MINA_ERR_STATE
int mb_pickles_statements_net_dev(mina_ctx *c, size_t batch, const mina_pickles_statements *s, uint32_t *d_pub, uint32_t *d_ok, const uint8_t *d_net);   // api_pickles.hip
int mb_kimchi_to_batch_net_dev(mina_ctx *c, size_t batch, uint32_t n_prev, uint32_t npub, const mb::KimchiIn &in, const mb::KimchiOut &out, uint32_t *d_bad, const uint8_t *d_net,
                               const void *pf_digest, uint32_t pf_stride, void *d_count);                                           // api_kimchi.hip

// ---- host-side worker pool (api_core.hip): persistent threads, created on first use -- min(hardware threads / 2, 64), $MINA_HOST_THREADS
// overrides.  A job is `n` independent items handed out in index order; `mb_pool_submit` returns at once (the boundary's pipeline parses
// chunk i + 1 while chunk i is on the GPU), `mb_pool_wait` joins in on the remaining items and returns when all are done.
struct MbPoolJob;
std::shared_ptr<MbPoolJob> mb_pool_submit(size_t n, std::function<void(size_t)> fn);
void mb_pool_wait(const std::shared_ptr<MbPoolJob> &job);
size_t mb_pool_threads();
// independent per-item host work (items are ~0.01 - 0.1 ms each: the pool only when there are enough of them)
template <class Fn> static inline void mb_parallel_for(size_t n, Fn fn) {
    if (n < 128 || mb_pool_threads() <= 1) { for (size_t i = 0; i < n; ++i) fn(i); return; }
    mb_pool_wait(mb_pool_submit(n, std::function<void(size_t)>(fn)));
}
// `n` bytes from the operating system's CSPRNG (getrandom(2), /dev/urandom as the fallback); false = none available: callers fail closed
bool mb_secure_random(void *buf, size_t n);

static inline int base_field_of(int curve) { return curve == CURVE_PALLAS ? FIELD_FP : FIELD_FQ; }
static inline int scalar_field_of(int curve) { return curve == CURVE_PALLAS ? FIELD_FQ : FIELD_FP; }
static inline bool bad_field(int f) { return f != 0 && f != 1; }

#define DISPATCH_FIELD(field, ...)                           \
    do { if ((field) == FIELD_FP) { constexpr int F_ = FIELD_FP; __VA_ARGS__; } else { constexpr int F_ = FIELD_FQ; __VA_ARGS__; } } while (0)
#define DISPATCH_CURVE(curve, ...)                           \
    do { if ((curve) == CURVE_PALLAS) { constexpr int C_ = CURVE_PALLAS; __VA_ARGS__; } else { constexpr int C_ = CURVE_VESTA; __VA_ARGS__; } } while (0)

// Runs `f(std::integral_constant<int, LN>{})` for the lane form LN = `lanes` (one of the rules above) and returns its result.  The template arguments list
// the forms the site instantiates kernels for; a form outside the list is an error, not a fall-back.
template <int LN, int... FORMS, class Fn> static inline int with_lanes(int lanes, Fn &&f) {
    if (lanes == LN) return f(std::integral_constant<int, LN>{});
    if constexpr (sizeof...(FORMS) > 0) return with_lanes<FORMS...>(lanes, std::forward<Fn>(f));
    else return fail(MINA_ERR_ARG, "no kernel of the " + std::to_string(lanes) + "-lane form at this site");
}

static inline uint32_t cdiv(size_t a, size_t b) { return (uint32_t)((a + b - 1) / b); }


// small host<->device helpers for the byte-buffer entry points
static inline int h2d(mina_ctx *c, DevBuf &b, const void *src, size_t bytes) {
    int rc = b.ensure(bytes ? bytes : 4);
    if (rc) return rc;
    if (bytes) HIPC(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->L->stream));
    return MINA_OK;
}
static inline int d2h_sync(mina_ctx *c, void *dst, const DevBuf &b, size_t bytes) {
    if (bytes) HIPC(hipMemcpyAsync(dst, b.p, bytes, hipMemcpyDeviceToHost, c->L->stream));
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(c->L->stream));
    return MINA_OK;
}

// The signed-digit recoding of the MSM has no window for a carry out of bit 255: scalars must be < 2^255 (every canonical field
// element is).  The host-buffer entry points reject anything else instead of returning a point that is off by 2^256 * P.
static inline bool scalars_below_2_255(const uint8_t *scalars, size_t n) { for (size_t i = 0; i < n; ++i) if (scalars[i * 32 + 31] & 0x80) return false; return true; }

void mb_prof_begin(mina_ctx *c, int stage);
void mb_prof_end(mina_ctx *c, int stage);
struct ProfScope {
    mina_ctx *c; int stage;
    ProfScope(mina_ctx *c_, int s_) : c(c_), stage(s_) { if (c->prof.mask & (1 << stage)) mb_prof_begin(c, stage); }
    ~ProfScope() { if (c->prof.mask & (1 << stage)) mb_prof_end(c, stage); }
};

// combined IPA opening check with inputs in HBM (api_ipa.hip)
namespace mb {
struct IpaShape { uint32_t batch, k, npts, ncomms, per; uint32_t override_slot = 0xffffffffu, expand_slot = 0xffffffffu;
                  uint32_t shared_lo = 0, shared_hi = 0, shared_h = 0, shared_expand0 = 0, nshared = 0;
                  uint32_t pow_first = 0; };   // per = 2k + ncomms + 4 points per proof
// pow_first: rho_b = rand_base^(b + pow_first), sigma_b = sg_rand_base^(b + pow_first).  0 = upstream's batch_verify (proof 0 has coefficient 1: fine when the
//   batch is ONE combination); 1 = the exchange variant (mina_state_job_fold_dev): the shards' partial sums are ADDED by the caller, so every coefficient of
//   every shard must be random -- G shards whose first proofs all carry coefficient 1 let two first proofs with discrepancies +tH / -tH cancel
// shared_*: list entries whose POINT is the same for every proof of the batch (the caller vouches: h, verifier-index commitments -- bits of
//   shared_lo/hi over the commitment index, ncomms <= 64 --, the index point of the expanded slot).  Their scalars are summed over the batch
//   first and enter the MSM ONCE, as `nshared` entries behind the per-proof lists (a third of a kimchi batch's 88 points per proof);
//   the per-proof entries keep a zero scalar (the MSM drops zero digits) and the real one in a side matrix (culprit search restores it)
// override_slot: commitment index whose point comes from `comm_override` (b*16 canonical words, e.g. the public-input commitment computed on the GPU)
// expand_slot: commitment index given as a linear combination instead of a point (kimchi's chunked ft commitment): its list entry becomes
//   IPA_EXPAND entries (point_j, weight * expand_sc[j]), so the combination is evaluated by the batch MSM; per grows by IPA_EXPAND - 1
static constexpr uint32_t IPA_EXPAND = 8;
struct IpaExpand {    // point 0 = *p0 (Montgomery, trusted index data), points 1..7 = pts + b*7*16 (canonical words, checked); scalars sc[b*stride + j] (Montgomery)
    const affine_t *p0 = nullptr; const uint32_t *pts = nullptr; const fe_t *sc = nullptr; uint32_t stride = 0;
};
struct IpaDevIn {     // structure-of-arrays over the batch, canonical little-endian words; layouts as in mina_ipa_opening
    const uint32_t *state /* b*24 */, *pos /* b*2 */, *cip /* b*8 */, *lr /* b*2k*16 */, *delta /* b*16 */, *sg /* b*16 */, *z1, *z2 /* b*8 */,
                   *pts /* b*npts*8 */, *r /* b*8 */, *xi /* b*8 */, *comms /* b*ncomms*16 */, *comm_override /* b*16 or null */, *rb /* 8 */, *sb /* 8 */;
    IpaExpand expand;
};
}
int mb_ipa_batch_check_dev(mina_ctx *c, int curve, mb::IpaShape sh, const mb::IpaDevIn &in, uint32_t *d_verdict /* [0] verdict, [1] malformed flag */, const FoldExport *fx = nullptr);
int mb_ipa_recheck_rows(mina_ctx *c, size_t lo, size_t cnt, uint32_t *d_verdict /* [0] verdict */);   // folded check of proofs [lo, lo + cnt) of the batch prepared last, from its rows; on the current lane
// The grouped culprit search's checks: `np` parts [lo[p], lo[p] + cnt[p]) (host arrays, proofs) in ONE pass on the current lane -- segmented fold, the fixed-base
// MSM with one problem per part, the segmented variable-base MSM, one comparison launch; d_flags[p] = 1 iff part p's folded check holds.  Nothing waits for the GPU.
// rows: from the rows of the opening check prepared last (as mb_ipa_recheck_rows).  accumulator: mb_accumulator_parts_prepare once per search (challenges,
// checked points, one malformed word per proof -- a part holding a malformed commitment fails), then any number of passes.
int mb_ipa_recheck_rows_parts(mina_ctx *c, size_t np, const uint32_t *lo, const uint32_t *cnt, uint32_t *d_flags, size_t stage_off /* this pass's MB_PARTS_STAGE * np bytes of the lane's pinned staging buffer */);
static constexpr size_t MB_PARTS_STAGE = 20;   // bytes per part of a pass's tables: [begin | end] in proofs, [begin | end] in row entries, the fold's matrix-core segment ids
int mb_accumulator_parts_prepare(mina_ctx *c, int curve, uint32_t k, size_t batch, const uint32_t *d_prechal, const uint32_t *d_sg_words);
int mb_accumulator_check_parts(mina_ctx *c, int curve, uint32_t k, size_t batch, const uint32_t *d_rho, size_t np, const uint32_t *lo, const uint32_t *cnt, uint32_t *d_flags, size_t stage_off);
size_t mb_search_parts_cap(mina_ctx *c, int curve, uint32_t k);      // parts per pass: min(128, 2^28 / (2^k * W)) for the SRS table's W windows
int mb_accumulator_check_dev(mina_ctx *c, int curve, uint32_t k, size_t batch, const uint32_t *d_prechal, const uint32_t *d_sg_words, const uint32_t *d_rho, uint32_t *d_verdict, const FoldExport *fx = nullptr);

// cross-file entry points (C++ linkage)
struct xyzz_dev;   // opaque: mb::xyzz_t in HBM
// fixed-base MSM over the SRS table of `curve`; writes the 17-word affine record and/or the XYZZ value
int mb_msm_fixed(mina_ctx *c, int curve, uint32_t n, const uint32_t *d_scalars, uint32_t *d_out_words, void *d_out_xyzz, uint32_t first = 0);
// variable-base MSM over Montgomery affine points already in HBM
// K2 fold on the current lane (no lane switch)
int mb_msm_table(mina_ctx *c, int curve, const void *d_table, uint32_t stride, uint32_t cbits, uint32_t W, uint32_t first, uint32_t n,
                 uint32_t nprob, const uint32_t *d_scalars, uint32_t *d_out_words, void *d_out_xyzz);
int mb_bpoly_single_from_prechallenges(mina_ctx *c, int field, uint32_t k, const uint32_t *d_prechal, uint32_t *d_out, uint32_t count);
int mb_bpoly_fold(mina_ctx *c, int field, uint32_t k, size_t batch, const uint32_t *d_chals, const uint32_t *d_weights, uint32_t *d_out);
int mb_msm_variable(mina_ctx *c, int curve, uint32_t n, const uint32_t *d_scalars, const void *d_points_mont,
                    uint32_t *d_out_words, void *d_out_xyzz);
// the segment tables of mina_msm_segments_dev / mina_b_poly_fold_segments_dev, read back on the current lane (one host wait) and checked against `limit` (api_msm.hip)
int mb_read_segments(mina_ctx *c, size_t nseg, const void *d_begin, const void *d_end, size_t limit, uint32_t *max_len, std::vector<uint32_t> *lens = nullptr /* the length of every segment */);
// the segmented forms on the current lane, tables already checked (max_len = the longest segment); the MSM takes Montgomery affine points and writes 17-word
// records and / or XYZZ values, one per segment.  mb_msm_segments_fit: the pipeline's limits hold for nseg segments of up to max_len entries
bool mb_msm_segments_fit(uint32_t max_len, size_t nseg);
int mb_msm_segments(mina_ctx *c, int curve, uint32_t n_total, size_t nseg, uint32_t max_len, const uint32_t *d_begin, const uint32_t *d_end,
                    const uint32_t *d_scalars, const void *d_points_mont, uint32_t *d_out_words, void *d_out_xyzz);
// Which kernels fold which segments of a segmented b_poly fold, decided on the HOST from the segments' lengths (both callers know them: mb_read_segments, the
// search's cnt[]).  mb_bpoly_seg_plan applies the rule -- matrix cores (bpoly_mfma_seg.cuh) where mina_verify_tuning.bpoly_mfma != 0, k >= 2 and
// mina_ctx::seg_fold_mfma_min <= length < 2^17; the VALU kernels (bpoly_seg.cuh) for every other segment, empty ones included -- and writes the ids of the
// matrix-core segments, ascending, to ids_host[0 .. n_mfma).  The caller uploads that list with its tables (no host wait) and sets d_ids before the fold.
struct BpolySegPlan {
    uint32_t mfma_min = 0;             // the rule the device kernels share: segments with mfma_min <= length < 2^17 are the matrix cores'; 0 = none
    uint32_t n_mfma = 0, n_valu = 0;   // matrix-core segments; non-empty VALU segments (empty ones count in neither)
    uint32_t max_mfma_len = 0, max_valu_len = 0;
    const uint32_t *d_ids = nullptr;   // device: n_mfma segment ids
};
BpolySegPlan mb_bpoly_seg_plan(const mina_ctx *c, uint32_t k, size_t nseg, const uint32_t *len, uint32_t *ids_host);
int mb_bpoly_fold_segments(mina_ctx *c, int field, uint32_t k, size_t batch, size_t nseg, const BpolySegPlan &plan, const uint32_t *d_begin, const uint32_t *d_end,
                           const uint32_t *d_chals, const uint32_t *d_weights, uint32_t *d_out);
