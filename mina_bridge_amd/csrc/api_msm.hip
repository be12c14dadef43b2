// api_msm.hip -- K1 host driver: queues the MSM kernel pipeline of msm.cuh on the context stream.
#include "ctx.h"
#include "msm.cuh"
#include "msm_seg.cuh"
#include <vector>

// ------------------------------------------------------------------------------------------------
// MSM driver: run_msm = plan (every decision and count) -> reserve (the workspace the plan needs) -> five stages (the launches)
static MsmShape fixed_shape(const SrsState &s, uint32_t first, uint32_t n) {
    MsmShape sh; sh.n = n; sh.c = s.c; sh.W = s.W; sh.NB = 1u << (s.c - 1); sh.nsets = 1; sh.table_stride = s.depth; sh.base_first = first; sh.nprob = 1; return sh;
}
static MsmShape variable_shape(uint32_t n) {
    MsmShape sh; sh.n = n;
    // window widths whose TOP window is not degenerate for 255-bit scalars: c = 8 (top digit < 64), 13 (W = 20, top digit
    // < 128), 15 (W = 18, the 18th window is always empty); c = 11 / 14 put a quarter of a window's entries in one bucket
    sh.c = n < 2048 ? 8 : (n < (1u << 17) ? 13 : 15);
    sh.W = (256 + sh.c - 1) / sh.c; sh.NB = 1u << (sh.c - 1); sh.nsets = sh.W; sh.table_stride = 0; sh.base_first = 0; sh.nprob = 1; return sh;
}

// the group law of the accumulate kernels: 8 x 32-bit words on the points themselves, or 29-bit limbs (ec29.cuh) on the points' 2^261-domain twin
// (SrsState::table29, MsmWorkspace::points29) or on its pre-split form (SrsState::table29s, tab29_t records)
enum MsmLaw { LAW_8X32, LAW_TWIN, LAW_SPLIT };

struct MsmPlan {
    MsmShape sh; SortShape ss;
    bool part_sort;       // partitioned LDS sort; false: the atomic counting sort
    bool bucket_lanes;    // accumulate with one lane per pair of count-ranked buckets (K1t); false: tasks of <= 8 entries and their 128-B partials
    MsmLaw law;
    bool red29;           // msm_fp29 = 3: the buckets of the multi-MSM form stay on 29-bit limbs and the 2-D reduction runs on them too
    bool pipelined;       // several lanes in flight: the throughput forms of the bucket sums and of the reduction
    bool coop;            // one MSM at a time: the reduction's latency form (four lanes per add)
    bool fused_finish;    // one bucket set per problem and no affine output wanted: the reduction kernel's result IS the answer (no finish launch)
    bool fused_tail;      // mina_ctx_set_msm_fused_tail on a task-form plan: stages 3 - 5 are ONE launch (msm.cuh msm_tail_kernel), whatever the sort, the law, `pipelined` or segments
    uint32_t nb_total; size_t entries, max_tasks; uint64_t gh_words;
    uint32_t R, C, log2C, seg_blocks, Gr, Gc; SegSum rows, cols;      // 2-D bucket reduction: C = 128 columns, R = NB / C rows (NB is a power of two in [128, 32768])
};

static int msm_plan(const MsmShape &sh, int nlanes, uint32_t fp29, bool twin, bool split_table /* the 29-bit tables the caller passed */, bool want_words, bool want_xyzz /* the outputs it wants */, bool fused_tail_mode /* mina_ctx::msm_fused_tail */, MsmPlan &p) {
    if (sh.nprob == 0 || sh.nsets % sh.nprob) return fail(MINA_ERR_ARG, "bad problem count");
    if ((uint64_t)sh.NB * sh.nsets > (1u << 26) || (uint64_t)sh.n * sh.W * sh.nprob > (1u << 28)) return fail(MINA_ERR_ARG, "MSM batch too large for one pipeline");
    if (sh.NB < 128 || sh.NB > 32768) return fail(MINA_ERR_ARG, "unsupported bucket count");
    p.sh = sh;
    p.nb_total = sh.NB * sh.nsets;
    p.entries = (size_t)sh.n * sh.W * sh.nprob;
    p.max_tasks = p.entries / MSM_TASK_LEN + p.nb_total + 1;
    // sort plan: partitioned LDS sort when the partition table fits (P <= 1024 with <= 2048 buckets per partition),
    // else the atomic counting sort
    SortShape &ss = p.ss; ss.fbits = 8; ss.Gl = cdiv(sh.n, 256); ss.SB = sh.NB * (sh.nsets / sh.nprob);
    while (ss.fbits < 11 && cdiv(ss.SB, 1u << ss.fbits) > 256) ++ss.fbits;
    ss.Pl = cdiv(ss.SB, 1u << ss.fbits);
    p.gh_words = (uint64_t)ss.Pl * ss.Gl * sh.nprob;
    p.part_sort = ss.Pl <= 1024 && p.gh_words <= (1u << 22);
    // throughput form of the accumulate (one lane per pair of count-ranked buckets, K1t) when one launch carries enough
    // buckets to fill the chip; a single MSM's 32768 buckets would leave it latency-bound (16 pipelined lanes: 6.2 k
    // proofs/s against 7.6 k with tasks)
    p.bucket_lanes = p.part_sort && sh.nprob >= 4;                                        // >= 64 k lanes of ~62 adds each
    p.law = !twin || !fp29 ? LAW_8X32 /* msm_fp29 = 0, the cross-check switch: the 8 x 32 law everywhere */ : (split_table && fp29 == 2 ? LAW_SPLIT : LAW_TWIN);
    p.red29 = p.bucket_lanes && p.law == LAW_TWIN && fp29 == 3;
    p.pipelined = nlanes > 1;
    p.coop = !p.pipelined && !p.red29;                         // one MSM at a time: latency form; pipelined lanes: throughput form (the 29-bit reduction has the throughput form only)
    p.fused_finish = sh.nsets == sh.nprob && !want_words && want_xyzz;
    p.fused_tail = fused_tail_mode && !p.bucket_lanes;         // (the bucket-lane form, and with it the 29-bit reduction, keeps the staged tail)
    p.C = 128; p.log2C = 7; p.R = sh.NB / p.C;
    SegSum &rows = p.rows, &cols = p.cols;
    const uint32_t chunk = p.coop ? SEG_CHUNK : 16, lpg = p.coop ? 4 : 1;
    rows.nseg = p.R * sh.nsets; rows.per_set = p.R; rows.len = p.C; rows.seg_stride = p.C; rows.elem_stride = 1; rows.lanes = p.C / chunk;
    cols.nseg = p.C * sh.nsets; cols.per_set = p.C; cols.len = p.R; cols.seg_stride = 1; cols.elem_stride = p.C;
    { uint32_t l = 1; while (l * chunk < p.R && l < 16) l <<= 1; cols.lanes = l; }   // workers per column, <= 16 (one wave even in the quad form)
    const uint32_t threads_rows = rows.nseg * rows.lanes * lpg, threads_cols = cols.nseg * cols.lanes * lpg;
    p.seg_blocks = cdiv(threads_rows > threads_cols ? threads_rows : threads_cols, 256);
    p.Gr = (p.R + 15) / 16; p.Gc = p.C / 16;
    return MINA_OK;
}

// the fused tail's ticket words, one per bucket set and one per problem: a block of whole 16-byte units at the start of its allocation, zeroed before every launch
static size_t tail_ticket_bytes(const MsmPlan &p) { return (((size_t)p.sh.nsets + p.sh.nprob) * 4 + 15) & ~(size_t)15; }

// every buffer of the lane's workspace the plan's launches touch, at the size they need (0: not on this plan's path)
static int msm_reserve(MsmWorkspace &w, const MsmPlan &p) {
    const size_t e = p.entries, nb = p.nb_total, t = p.max_tasks, sets = p.sh.nsets, xz = sizeof(xyzz_t);
    const bool atomic = !p.part_sort, tasks = !p.bucket_lanes;            // tasks: task numbering and the 128-B task partials
    const size_t staged = p.fused_tail ? 0 : 1, fused = p.fused_tail ? 1 : 0;   // the staged tail's buckets and reduction arrays | the fused tail's row pairs and tickets
    const struct { DevBuf &buf; size_t bytes; } need[] = {
        {w.ghist, p.part_sort ? (p.gh_words + 8) * 4 : 0}, {w.stage, p.part_sort ? e * 8 : 0}, {w.ekey, e * 4}, {w.eval, atomic ? e * 4 : 0}, {w.eoff, atomic ? e * 4 : 0},
        {w.sorted, e * 4}, {w.count, nb * 4}, {w.start, (nb + 1) * 4},
        {w.order, p.bucket_lanes ? nb * 4 : 0}, {w.buckets29, p.red29 ? nb * sizeof(xyzz29_t) : 0}, {w.seg_bad, p.red29 ? ((size_t)(p.sh.NB / 128) + 128) * sets * 4 : 0},
        {w.task_start, tasks ? (nb + 1) * 4 : 0}, {w.rem_pos, tasks ? nb * 4 : 0}, {w.rem_bucket, tasks ? nb * 4 : 0}, {w.partial, tasks ? t * xz : 0},
        {w.info, 16}, {w.redo, p.law != LAW_8X32 ? (std::max(t, nb) + 1) * 4 : 0}, {w.heavy, (t / MSM_HEAVY_TASKS + e / MSM_HEAVY_ENTRIES + 2) * 4}, {w.buckets, staged * nb * xz},
        {w.red_r, staged * p.R * sets * xz}, {w.red_ws, staged * p.C * sets * xz}, {w.red2_r, staged * 24 * sets * xz}, {w.red2_w, staged * 24 * sets * xz}, {w.set_total, sets * xz},
        {w.tail_rows, fused * 2 * p.R * sets * xz}, {w.tail_tickets, fused * tail_ticket_bytes(p)}};
    for (const auto &n : need) if (int rc = n.buf.ensure(n.bytes)) return rc;
    return MINA_OK;
}

// runs f(std::true_type{}) or f(std::false_type{}): a kernel's two template forms at ONE launch expression
template <class Fn> static inline void with_form(bool b, Fn &&f) { if (b) f(std::true_type{}); else f(std::false_type{}); }

// one call's launches: the five stages, in the order run_msm calls them, over the plan, the lane's workspace and stream and the base field's constants
template <int F>
struct MsmRun {
    mina_ctx *c; const MsmPlan &p; MsmWorkspace &w; hipStream_t st; const FieldK &fk; bool gcd_inverse;      // gcd_inverse: mina_ctx::fast_inverse when the call was queued
    // one pass of the partitioned sort's level 1 (K1p-a counts, K1p-c scatters into the staging array), over segments or over problems of sh.n scalars
    template <bool SCATTER> void part_pass(const uint32_t *d_scalars, const MsmSegments *seg) {
        const uint32_t grid = p.ss.Gl * p.sh.nprob;
        uint2 *staging = SCATTER ? w.stage.as<uint2>() : nullptr;
        if (seg) msm_part_seg_kernel<SCATTER><<<grid, 1024, 0, st>>>(p.sh, p.ss, *seg, d_scalars, w.ghist.as<uint32_t>(), staging, w.ekey.as<uint32_t>());
        else msm_part_kernel<SCATTER><<<grid, 1024, 0, st>>>(p.sh, p.ss, d_scalars, w.ghist.as<uint32_t>(), staging, w.ekey.as<uint32_t>());
    }

    // the task form's bucket scan (K1b) and the inverse of its remainder ranks (K1b'), behind either sort
    void scan_tasks() {
        msm_scan_kernel<<<1, 1024, 0, st>>>(p.nb_total, w.count.as<uint32_t>(), w.start.as<uint32_t>(), w.task_start.as<uint32_t>(), w.rem_pos.as<uint32_t>(), w.info.as<uint32_t>());
        msm_rem_invert_kernel<<<cdiv(p.nb_total, 256), 256, 0, st>>>(p.nb_total, w.rem_pos.as<uint32_t>(), w.rem_bucket.as<uint32_t>());
    }

    // stage 1: digits -> point references in bucket order (`sorted`, `start`), and the accumulate's work list (bucket order | tasks)
    int sort(const uint32_t *d_scalars, const MsmSegments *seg) {
        if (p.part_sort) {
            { ProfScope ps_(c, PS_DIGITS);
              part_pass<false>(d_scalars, seg);
              msm_excl_scan_kernel<<<1, 1024, 0, st>>>((uint32_t)p.gh_words, w.ghist.as<uint32_t>()); }
            { ProfScope ps_(c, PS_SCATTER);
              part_pass<true>(d_scalars, seg);
              msm_part_sort_kernel<<<p.ss.Pl * p.sh.nprob, 1024, 0, st>>>(p.ss, w.ghist.as<uint32_t>(), w.stage.as<uint2>(), w.count.as<uint32_t>(), w.sorted.as<uint32_t>(), w.info.as<uint32_t>()); }
            ProfScope ps_(c, PS_SCAN);
            if (p.bucket_lanes) msm_order_kernel<<<p.sh.nprob, 1024, 0, st>>>(p.ss, p.sh.nprob, w.ghist.as<uint32_t>(), w.count.as<uint32_t>(), w.start.as<uint32_t>(), w.order.as<uint32_t>(), w.info.as<uint32_t>(), w.heavy.as<uint32_t>());
            else scan_tasks();
            return MINA_OK;
        }
        HIPC(hipMemsetAsync(w.count.p, 0, (size_t)p.nb_total * 4, st));
        { ProfScope ps_(c, PS_DIGITS);
          if (seg) msm_digits_seg_kernel<<<cdiv(p.entries, 256), 256, 0, st>>>(p.sh, *seg, d_scalars, w.count.as<uint32_t>(), w.ekey.as<uint32_t>(), w.eval.as<uint32_t>(), w.eoff.as<uint32_t>());
          else msm_digits_kernel<<<cdiv(p.entries, 256), 256, 0, st>>>(p.sh, d_scalars, w.count.as<uint32_t>(), w.ekey.as<uint32_t>(), w.eval.as<uint32_t>(), w.eoff.as<uint32_t>()); }
        { ProfScope ps_(c, PS_SCAN); scan_tasks(); }
        ProfScope ps_(c, PS_SCATTER);
        msm_scatter_kernel<<<cdiv(p.entries, 256), 256, 0, st>>>(p.entries, w.ekey.as<uint32_t>(), w.eval.as<uint32_t>(), w.eoff.as<uint32_t>(), w.start.as<uint32_t>(), w.sorted.as<uint32_t>());
        return MINA_OK;
    }

    // stage 2: sums per bucket (bucket lanes) or per task; d_tab29 = the table of p.law (null: the 8 x 32 law).  What the 29-bit kernels hand back -- equal / opposite
    // points, none on SRS points with unstructured scalars -- goes through the 8 x 32 law's redo queue.
    void accumulate(const affine_t *d_points, const void *d_tab29) {
        ProfScope ps_(c, PS_ACCUMULATE);
        if (p.bucket_lanes) {
            const uint32_t grid = cdiv(p.nb_total / 2, 256);
            if (p.law == LAW_8X32) { msm_accumulate_bucket_kernel<F><<<grid, 256, 0, st>>>(p.nb_total, p.ss.SB, w.start.as<uint32_t>(), w.order.as<uint32_t>(), w.sorted.as<uint32_t>(), d_points, fk.one, w.buckets.as<xyzz_t>()); return; }
            with_form(p.law == LAW_SPLIT, [&](auto split) {
                msm_accumulate_bucket29_kernel<F, decltype(split)::value ? 2 : 1><<<grid, 256, 0, st>>>(p.nb_total, p.ss.SB, w.start.as<uint32_t>(), w.order.as<uint32_t>(), w.sorted.as<uint32_t>(), d_tab29, fk.one, fk.m32,
                                                                                                       w.buckets.as<xyzz_t>(), w.info.as<uint32_t>(), w.redo.as<uint32_t>(), p.red29 ? w.buckets29.as<xyzz29_t>() : nullptr); });
            // the redo launch is sized by the bucket count (grid-stride over info[3]; lanes beyond it leave at once): a batch of repeated commitments may hand every bucket
            // back, and 16 blocks -- the size until round 6 -- would have summed them on 1024 lanes
            msm_bucket_redo_kernel<F><<<std::min<uint32_t>(1024u, cdiv(p.nb_total, 64)), 64, 0, st>>>(w.start.as<uint32_t>(), w.info.as<uint32_t>(), w.redo.as<uint32_t>(), w.sorted.as<uint32_t>(), d_points, fk.one, w.buckets.as<xyzz_t>());
            return;
        }
        const uint32_t grid = cdiv(p.max_tasks, 256);
        if (p.law != LAW_8X32)
            with_form(p.law == LAW_SPLIT, [&](auto split) {
                msm_accumulate29_kernel<F, decltype(split)::value ? 2 : 1><<<grid, 256, 0, st>>>(p.nb_total, w.start.as<uint32_t>(), w.task_start.as<uint32_t>(), w.rem_bucket.as<uint32_t>(), w.info.as<uint32_t>(),
                                                                                                w.sorted.as<uint32_t>(), d_tab29, fk.one, fk.m32, w.partial.as<xyzz_t>(), w.info.as<uint32_t>(), w.redo.as<uint32_t>()); });
        // behind the 29-bit kernel: the tasks handed back (none on SRS points), the 8 x 32 kernel over the redo queue -- a full-size launch whose lanes beyond info[3] leave at once
        msm_accumulate_kernel<F><<<grid, 256, 0, st>>>(p.nb_total, w.start.as<uint32_t>(), w.task_start.as<uint32_t>(), w.rem_bucket.as<uint32_t>(), w.info.as<uint32_t>(),
                                                      w.sorted.as<uint32_t>(), d_points, fk.one, w.partial.as<xyzz_t>(), p.law != LAW_8X32 ? w.redo.as<uint32_t>() : nullptr);
    }

    // stage 3: what stage 2 left out of `buckets`: the heavy buckets, and in the task form every bucket = the sum of its task partials
    void bucket_sums(const affine_t *d_points) {
        ProfScope ps_(c, PS_BUCKET_SUM);
        if (p.bucket_lanes) {
            msm_bucket_heavy_entries_kernel<F><<<128, 256, 0, st>>>(w.start.as<uint32_t>(), w.info.as<uint32_t>(), w.heavy.as<uint32_t>(), w.sorted.as<uint32_t>(), d_points, fk.one, w.buckets.as<xyzz_t>());
            // the buckets the two 8 x 32 kernels wrote join the others on 29-bit limbs (none on SRS points with unstructured scalars: a fixed-size launch that finds empty lists)
            if (p.red29) msm_buckets_to29_kernel<F><<<16, 64, 0, st>>>(w.info.as<uint32_t>(), w.heavy.as<uint32_t>(), w.redo.as<uint32_t>(), w.buckets.as<xyzz_t>(), fk.m32, w.buckets29.as<xyzz29_t>());
            return;
        }
        if (p.pipelined)
            msm_bucket_sum_lane_kernel<F><<<cdiv(p.nb_total, 256), 256, 0, st>>>(p.nb_total, w.task_start.as<uint32_t>(), w.rem_pos.as<uint32_t>(), w.info.as<uint32_t>(), w.partial.as<xyzz_t>(), w.buckets.as<xyzz_t>(), w.heavy.as<uint32_t>());
        else
            msm_bucket_sum_kernel<F><<<cdiv((size_t)p.nb_total * 4, 256), 256, 0, st>>>(p.nb_total, w.task_start.as<uint32_t>(), w.rem_pos.as<uint32_t>(), w.info.as<uint32_t>(), w.partial.as<xyzz_t>(), w.buckets.as<xyzz_t>(), w.heavy.as<uint32_t>());
        msm_bucket_sum_heavy_kernel<F><<<128, 256, 0, st>>>(w.task_start.as<uint32_t>(), w.rem_pos.as<uint32_t>(), w.info.as<uint32_t>(), w.partial.as<xyzz_t>(), w.buckets.as<xyzz_t>(), w.heavy.as<uint32_t>());
    }

    // stage 4: the 2-D bucket reduction, one total per bucket set; d_fused (p.fused_finish): the totals are the results and leave here
    int reduce(xyzz_t *d_fused) {
        { ProfScope ps_(c, PS_REDUCE_A);
          if (p.red29) {
              const uint32_t nseg = p.rows.nseg + p.cols.nseg;
              HIPC(hipMemsetAsync(w.seg_bad.p, 0, (size_t)nseg * 4, st));
              msm_segsum29_kernel<F><<<dim3(p.seg_blocks, 2), 256, 0, st>>>(p.sh.NB, p.rows, p.cols, w.buckets29.as<xyzz29_t>(), fk.one, w.red_r.as<xyzz_t>(), w.red_ws.as<xyzz_t>(), w.seg_bad.as<uint32_t>());
              msm_segsum29_redo_kernel<F><<<cdiv(nseg, 64), 64, 0, st>>>(p.sh.NB, p.rows, p.cols, w.buckets29.as<xyzz29_t>(), fk.one, w.red_r.as<xyzz_t>(), w.red_ws.as<xyzz_t>(), w.seg_bad.as<uint32_t>());
          }
          else with_form(p.coop, [&](auto coop) {
              msm_segsum_kernel<F, decltype(coop)::value><<<dim3(p.seg_blocks, 2), 256, 0, st>>>(p.sh.NB, p.rows, p.cols, w.buckets.as<xyzz_t>(), w.red_r.as<xyzz_t>(), w.red_ws.as<xyzz_t>()); }); }
        ProfScope ps_(c, PS_REDUCE_BC);
        msm_wsum16_kernel<F><<<dim3(p.Gr + p.Gc, p.sh.nsets), 64, 0, st>>>(p.R, p.C, p.Gr, w.red_r.as<xyzz_t>(), w.red_ws.as<xyzz_t>(), w.red2_r.as<xyzz_t>(), w.red2_w.as<xyzz_t>());
        msm_reduce2d_kernel<F><<<p.sh.nsets, 256, 0, st>>>(p.Gr, p.Gc, p.log2C, w.red2_r.as<xyzz_t>(), w.red2_w.as<xyzz_t>(), w.set_total.as<xyzz_t>(), d_fused);
        return MINA_OK;
    }

    // stage 5: a problem's set totals -> its result, affine record and / or XYZZ; gcd_inverse (mina_ctx_set_fast_inverse): the kernel whose inversion is fe_modinv.cuh's
    void finish(uint32_t *d_out_words, xyzz_t *d_out_xyzz) {
        ProfScope ps_(c, PS_FINISH);
        if (gcd_inverse) msm_finish_gcd_kernel<F><<<p.sh.nprob, 64, 0, st>>>(p.sh.nsets / p.sh.nprob, p.sh.c, w.set_total.as<xyzz_t>(), fk.r2, d_out_xyzz, d_out_words);
        else msm_finish_kernel<F><<<p.sh.nprob, 64, 0, st>>>(p.sh.nsets / p.sh.nprob, p.sh.c, w.set_total.as<xyzz_t>(), fk.one, fk.pm2, d_out_xyzz, d_out_words);
    }

    // stages 3 - 5 of a p.fused_tail plan in one launch: a workgroup per row of 128 buckets; the last arriver of a set totals it, the last of a problem finishes it.
    // The tickets are zeroed in stream order ahead of every launch: a run that failed leaves nothing behind for the next.
    int tail(uint32_t *d_out_words, xyzz_t *d_out_xyzz) {
        ProfScope ps_(c, PS_BUCKET_SUM);
        HIPC(hipMemsetAsync(w.tail_tickets.p, 0, tail_ticket_bytes(p), st));
        if (gcd_inverse)
            msm_tail_gcd_kernel<F><<<p.R * p.sh.nsets, 256, 0, st>>>(p.R, p.sh.nsets, p.sh.nsets / p.sh.nprob, p.sh.c, w.task_start.as<uint32_t>(), w.rem_pos.as<uint32_t>(), w.info.as<uint32_t>(), w.partial.as<xyzz_t>(),
                                                                     w.tail_rows.as<xyzz_t>(), w.tail_tickets.as<uint32_t>(), w.set_total.as<xyzz_t>(), fk.r2, d_out_xyzz, d_out_words);
        else
            msm_tail_kernel<F><<<p.R * p.sh.nsets, 256, 0, st>>>(p.R, p.sh.nsets, p.sh.nsets / p.sh.nprob, p.sh.c, w.task_start.as<uint32_t>(), w.rem_pos.as<uint32_t>(), w.info.as<uint32_t>(), w.partial.as<xyzz_t>(),
                                                                 w.tail_rows.as<xyzz_t>(), w.tail_tickets.as<uint32_t>(), w.set_total.as<xyzz_t>(), fk.one, fk.pm2, d_out_xyzz, d_out_words);
        return MINA_OK;
    }
};

template <int F>
static int run_msm(mina_ctx *c, const MsmShape &sh, const uint32_t *d_scalars, const affine_t *d_points,
                   uint32_t *d_out_words /* 17 words per problem */, xyzz_t *d_out_xyzz /* one per problem */,
                   const affine_t *d_points29 = nullptr /* the table's 2^261-domain twin (SrsState::table29): the accumulate kernels then run on 29-bit limbs (ec29.cuh) */,
                   const void *d_points29s = nullptr /* ... or its pre-split form (SrsState::table29s, tab29_t records; mina_verify_tuning.msm_fp29 = 2) */,
                   const MsmSegments *seg = nullptr /* the problems are ranges of ONE scalar / point array (msm_seg.cuh): sh.n = the longest range, `d_scalars` and the references index the whole array */) {
    MsmPlan p;
    if (int rc = msm_plan(sh, c->nlanes, mb_tune().msm_fp29, d_points29 != nullptr, d_points29 && d_points29s, d_out_words != nullptr, d_out_xyzz != nullptr, c->msm_fused_tail, p)) return rc;
    if (int rc = msm_reserve(c->L->ws, p)) return rc;
    MsmRun<F> run{c, p, c->L->ws, c->L->stream, c->fk[F], c->fast_inverse};
    if (int rc = run.sort(d_scalars, seg)) return rc;
    run.accumulate(d_points, p.law == LAW_SPLIT ? d_points29s : p.law == LAW_TWIN ? d_points29 : nullptr);
    if (p.fused_tail) { if (int rc = run.tail(d_out_words, d_out_xyzz)) return rc; }
    else {
        run.bucket_sums(d_points);
        if (int rc = run.reduce(p.fused_finish ? d_out_xyzz : nullptr)) return rc;
        if (!p.fused_finish) run.finish(d_out_words, d_out_xyzz);
    }
    HIPC(hipGetLastError());
    ++(p.fused_tail ? c->mt_fused_runs : c->mt_staged_runs);
    if (p.fused_tail || !p.fused_finish) ++(run.gcd_inverse ? c->inv_gcd_finishes : c->inv_fermat_finishes);      // a finish ran, in the tail kernel or on its own
    return MINA_OK;
}

int mb_msm_fixed(mina_ctx *c, int curve, uint32_t n, const uint32_t *d_scalars, uint32_t *d_out_words, void *d_out_xyzz, uint32_t first) {
    SrsState &s = c->srs[curve];
    if (s.depth == 0) return fail(MINA_ERR_STATE, "SRS not loaded for this curve");
    if (n == 0 || (uint64_t)first + n > s.depth) return fail(MINA_ERR_ARG, "base range must lie inside the SRS");
    int rc = MINA_OK;
    DISPATCH_FIELD(base_field_of(curve), { rc = run_msm<F_>(c, fixed_shape(s, first, n), d_scalars, s.table.as<affine_t>(), d_out_words, (xyzz_t *)d_out_xyzz, s.table29.as<affine_t>(), s.table29s.p); });
    return rc;
}

// nprob MSMs over one fixed-base window table (table[w * stride + i] = 2^(cbits w) * base_i): results per problem
int mb_msm_table(mina_ctx *c, int curve, const void *d_table, uint32_t stride, uint32_t cbits, uint32_t W, uint32_t first, uint32_t n,
                 uint32_t nprob, const uint32_t *d_scalars, uint32_t *d_out_words, void *d_out_xyzz) {
    if (n == 0 || nprob == 0 || (uint64_t)first + n > stride) return fail(MINA_ERR_ARG, "bad table MSM shape");
    MsmShape sh; sh.n = n; sh.c = cbits; sh.W = W; sh.NB = 1u << (cbits - 1); sh.nsets = nprob; sh.table_stride = stride; sh.base_first = first; sh.nprob = nprob;
    int rc = MINA_OK;
    const SrsState &s = c->srs[curve];
    const affine_t *t29 = (d_table == s.table.p && s.table29.p) ? (const affine_t *)s.table29.p : nullptr;      // the SRS table has a 2^261-domain twin; other tables do not
    DISPATCH_FIELD(base_field_of(curve), { rc = run_msm<F_>(c, sh, d_scalars, (const affine_t *)d_table, d_out_words, (xyzz_t *)d_out_xyzz, t29, s.table29s.p); });
    return rc;
}

// Round 5: the accumulate kernels run the 29-bit group law on variable bases too.  The points get a 2^261-domain twin first (two products per point against
// W = 20 mixed adds of ten products each: 1 %); equal / opposite points -- proofs may repeat a commitment -- are found exactly on the lazy limbs and go through
// the 8 x 32 redo queue like everywhere else.  mina_verify_tuning.msm_fp29 = 0: the 8 x 32 law (cross-check).
// Below 32 points per problem -- the part MSMs of a culprit search, single openings -- the twin's launch costs more than the 29-bit law saves: the 8 x 32 law, no
// twin, no redo queue.  *twin = the lane's points29, or null.
static int points_twin(mina_ctx *c, int curve, uint32_t n_points, uint32_t per_problem, const void *d_points_mont, const affine_t **twin) {
    *twin = nullptr;
    if (!mb_tune().msm_fp29 || per_problem < 32 || !n_points) return MINA_OK;
    MsmWorkspace &w = c->L->ws;
    if (int rc = w.points29.ensure((size_t)n_points * sizeof(affine_t))) return rc;
    DISPATCH_FIELD(base_field_of(curve), { msm_table29_kernel<F_><<<cdiv(n_points, 256), 256, 0, c->L->stream>>>(n_points, (const affine_t *)d_points_mont, c->fk[F_].m32, w.points29.as<affine_t>()); });
    *twin = w.points29.as<affine_t>();
    return MINA_OK;
}

// n canonical affine points in device memory -> Montgomery form in the lane's `points`, where the variable-base drivers read them
static int bases_to_mont(mina_ctx *c, int curve, size_t n, const void *d_bases) {
    MsmWorkspace &w = c->L->ws;
    if (int rc = w.points.ensure((n ? n : 1) * sizeof(affine_t))) return rc;
    if (n) DISPATCH_FIELD(base_field_of(curve), { points_to_mont_kernel<F_><<<cdiv(n, 256), 256, 0, c->L->stream>>>((uint32_t)n, (const uint32_t *)d_bases, c->fk[F_].r2, w.points.as<affine_t>()); });
    return MINA_OK;
}

int mb_msm_variable(mina_ctx *c, int curve, uint32_t n, const uint32_t *d_scalars, const void *d_points_mont,
                    uint32_t *d_out_words, void *d_out_xyzz) {
    if (n == 0) return fail(MINA_ERR_ARG, "n must be positive");
    int rc = MINA_OK;
    const affine_t *twin;
    if ((rc = points_twin(c, curve, n, n, d_points_mont, &twin))) return rc;
    DISPATCH_FIELD(base_field_of(curve), { rc = run_msm<F_>(c, variable_shape(n), d_scalars, (const affine_t *)d_points_mont, d_out_words, (xyzz_t *)d_out_xyzz, twin); });
    return rc;
}

// The segment tables of the two segmented entry points (device memory): read back on the current lane -- the one host wait of those calls, behind whatever
// the lane already holds -- and checked: begin <= end <= limit for every segment.  max_len = the longest segment.
int mb_read_segments(mina_ctx *c, size_t nseg, const void *d_begin, const void *d_end, size_t limit, uint32_t *max_len, std::vector<uint32_t> *lens) {
    std::vector<uint32_t> h(2 * nseg);
    HIPC(hipMemcpyAsync(h.data(), d_begin, nseg * 4, hipMemcpyDeviceToHost, c->L->stream));
    HIPC(hipMemcpyAsync(h.data() + nseg, d_end, nseg * 4, hipMemcpyDeviceToHost, c->L->stream));
    HIPC(hipStreamSynchronize(c->L->stream));
    uint32_t mx = 0;
    for (size_t s = 0; s < nseg; ++s) {
        const uint32_t b = h[s], e = h[nseg + s];
        if (e < b || e > limit) return fail(MINA_ERR_ARG, "segment " + std::to_string(s) + ": need begin <= end <= " + std::to_string(limit));
        mx = std::max(mx, e - b);
    }
    *max_len = mx;
    if (lens) { lens->resize(nseg); for (size_t s = 0; s < nseg; ++s) (*lens)[s] = h[nseg + s] - h[s]; }
    return MINA_OK;
}

// nseg variable-base MSMs over ranges of one point / scalar array: the ranges are the problems of ONE pipeline (msm_seg.cuh), within its two limits
static bool segments_fit(const MsmShape &v, size_t nseg) { return (uint64_t)v.NB * v.W * nseg <= (1u << 26) && (uint64_t)v.n * v.W * nseg <= (1u << 28); }

static int msm_segments_shape(uint32_t max_len, size_t nseg, MsmShape &sh) {
    sh = variable_shape(max_len ? max_len : 1);                  // every segment empty: one scalar slot per problem that no lane fills -> nseg times infinity
    if (!segments_fit(sh, nseg))
        return fail(MINA_ERR_ARG, "segmented MSM too large for one pipeline: need NB * W * nseg <= 2^26 and longest segment * W * nseg <= 2^28 (W windows of NB buckets: 32 x 128 below 2048 points per segment, 20 x 4096 below 2^17, 18 x 16384 above)");
    sh.nprob = (uint32_t)nseg; sh.nsets = sh.W * (uint32_t)nseg;
    return MINA_OK;
}

bool mb_msm_segments_fit(uint32_t max_len, size_t nseg) { return nseg > 0 && segments_fit(variable_shape(max_len ? max_len : 1), nseg); }

// on the current lane; the points are Montgomery affine already; max_len = the longest segment (the caller has read or made the tables)
int mb_msm_segments(mina_ctx *c, int curve, uint32_t n_total, size_t nseg, uint32_t max_len, const uint32_t *d_begin, const uint32_t *d_end,
                    const uint32_t *d_scalars, const void *d_points_mont, uint32_t *d_out_words, void *d_out_xyzz) {
    MsmShape sh;
    int rc;
    if ((rc = msm_segments_shape(max_len, nseg, sh))) return rc;
    const affine_t *twin;
    if ((rc = points_twin(c, curve, n_total, max_len, d_points_mont, &twin))) return rc;
    const MsmSegments sg{d_begin, d_end, n_total};
    DISPATCH_FIELD(base_field_of(curve), { rc = run_msm<F_>(c, sh, d_scalars, (const affine_t *)d_points_mont, d_out_words, (xyzz_t *)d_out_xyzz, twin, nullptr, &sg); });
    return rc;
}

extern "C" int mina_ctx_set_msm_fused_tail(mina_ctx *c, int on) {
    if (!c) return fail(MINA_ERR_ARG, "null argument");
    if (on != 0 && on != 1) return fail(MINA_ERR_ARG, "fused MSM tail: 0 (off) or 1 (on)");
    c->msm_fused_tail = on != 0;
    return MINA_OK;
}

extern "C" int mina_ctx_msm_tail_stats(mina_ctx *c, uint64_t *fused_runs, uint64_t *staged_runs) {
    if (!c || !fused_runs || !staged_runs) return fail(MINA_ERR_ARG, "null argument");
    *fused_runs = c->mt_fused_runs; *staged_runs = c->mt_staged_runs;
    return MINA_OK;
}

extern "C" int mina_ctx_set_fast_inverse(mina_ctx *c, int on) {
    if (!c) return fail(MINA_ERR_ARG, "null argument");
    if (on != 0 && on != 1) return fail(MINA_ERR_ARG, "fast inverse: 0 (off) or 1 (on)");
    c->fast_inverse = on != 0;
    return MINA_OK;
}

extern "C" int mina_ctx_inverse_stats(mina_ctx *c, uint64_t *gcd_finishes, uint64_t *fermat_finishes) {
    if (!c || !gcd_finishes || !fermat_finishes) return fail(MINA_ERR_ARG, "null argument");
    *gcd_finishes = c->inv_gcd_finishes; *fermat_finishes = c->inv_fermat_finishes;
    return MINA_OK;
}

// the chain inverse (ctx.h): which covered launch runs which form is decided where it is queued, by mina_ctx::gcd_launch()
extern "C" int mina_ctx_set_chain_inverse(mina_ctx *c, int on) {
    if (!c) return fail(MINA_ERR_ARG, "null argument");
    if (on != 0 && on != 1) return fail(MINA_ERR_ARG, "chain inverse: 0 (off) or 1 (on)");
    c->chain_inverse = on != 0;
    return MINA_OK;
}

extern "C" int mina_ctx_chain_inverse_stats(mina_ctx *c, uint64_t *gcd_launches, uint64_t *fermat_launches) {
    if (!c || !gcd_launches || !fermat_launches) return fail(MINA_ERR_ARG, "null argument");
    *gcd_launches = c->chain_gcd_launches; *fermat_launches = c->chain_fermat_launches;
    return MINA_OK;
}

extern "C" int mina_msm_segments_dev(mina_ctx *c, int curve, size_t n_total, size_t nseg, const void *d_seg_begin, const void *d_seg_end,
                                     const void *d_bases, const void *d_scalars, void *d_out) {
    if (!c || !d_seg_begin || !d_seg_end || !d_out || (n_total && (!d_bases || !d_scalars))) return fail(MINA_ERR_ARG, "null argument");
    if (curve != 0 && curve != 1) return fail(MINA_ERR_ARG, "bad curve");
    if (((uintptr_t)d_seg_begin | (uintptr_t)d_seg_end | (uintptr_t)d_out) & 3u) return fail(MINA_ERR_ARG, "segment tables and records are arrays of 32-bit words: 4-byte alignment");
    if (((uintptr_t)d_bases | (uintptr_t)d_scalars) & 15u) return fail(MINA_ERR_ARG, "bases and scalars are read 16 bytes at a time: 16-byte alignment");
    if (nseg == 0 || nseg > (1u << 19) || n_total > (1u << 24)) return fail(MINA_ERR_ARG, "bad nseg / n_total");
    MsmShape sh;
    if (int rc = msm_segments_shape(0, nseg, sh)) return rc;     // the bucket limit at the smallest window shape: refused before the device is touched
    HIPC(hipSetDevice(c->device));
    c->next_lane();
    uint32_t max_len = 0;
    if (int rc = mb_read_segments(c, nseg, d_seg_begin, d_seg_end, n_total, &max_len)) return rc;
    if (int rc = msm_segments_shape(max_len, nseg, sh)) return rc;
    if (int rc = bases_to_mont(c, curve, n_total, d_bases)) return rc;
    return mb_msm_segments(c, curve, (uint32_t)n_total, nseg, max_len, (const uint32_t *)d_seg_begin, (const uint32_t *)d_seg_end, (const uint32_t *)d_scalars, c->L->ws.points.p, (uint32_t *)d_out, nullptr);
}

extern "C" int mina_msm_dev(mina_ctx *c, int curve, size_t n, const void *d_bases, const void *d_scalars, void *d_out) {
    if (!c || !d_bases || !d_scalars || !d_out) return fail(MINA_ERR_ARG, "null argument");
    if (curve != 0 && curve != 1) return fail(MINA_ERR_ARG, "bad curve");
    if (n == 0 || n > (1u << 24)) return fail(MINA_ERR_ARG, "bad n");
    HIPC(hipSetDevice(c->device));
    c->next_lane();
    if (int rc = bases_to_mont(c, curve, n, d_bases)) return rc;
    return mb_msm_variable(c, curve, (uint32_t)n, (const uint32_t *)d_scalars, c->L->ws.points.p, (uint32_t *)d_out, nullptr);
}

extern "C" int mina_msm_srs_dev(mina_ctx *c, int curve, size_t n, const void *d_scalars, void *d_out) {
    if (!c || !d_scalars || !d_out) return fail(MINA_ERR_ARG, "null argument");
    if (curve != 0 && curve != 1) return fail(MINA_ERR_ARG, "bad curve");
    if (n > 0xffffffffu) return fail(MINA_ERR_ARG, "n too large");
    HIPC(hipSetDevice(c->device));
    c->next_lane();
    return mb_msm_fixed(c, curve, (uint32_t)n, (const uint32_t *)d_scalars, (uint32_t *)d_out, nullptr);
}

extern "C" int mina_msm_srs_range_dev(mina_ctx *c, int curve, uint32_t first, size_t n, const void *d_scalars, void *d_out) {
    if (!c || !d_scalars || !d_out) return fail(MINA_ERR_ARG, "null argument");
    if (curve != 0 && curve != 1) return fail(MINA_ERR_ARG, "bad curve");
    if (n == 0 || n > 0xffffffffu) return fail(MINA_ERR_ARG, "bad n");
    HIPC(hipSetDevice(c->device));
    c->next_lane();
    return mb_msm_fixed(c, curve, (uint32_t)n, (const uint32_t *)d_scalars, (uint32_t *)d_out, nullptr, first);
}

// ------------------------------------------------------------------------------------------------
// the host-buffer entry points: nprob problems of n scalars each in, nprob 64-byte points out (zeros = infinity), on lane 0, waiting for the result
// What they refuse alike, in their common order: null arguments (`inputs`: the arrays a call with work to do reads), the curve; then the call with nothing to
// add up -- nprob times infinity, *done set.
static int host_msm_enter(mina_ctx *c, int curve, size_t n, size_t nprob, bool inputs, uint8_t *out, bool *done) {
    *done = false;
    if (!c || !out || (n && nprob && !inputs)) return fail(MINA_ERR_ARG, "null argument");
    if (curve != 0 && curve != 1) return fail(MINA_ERR_ARG, "bad curve");
    if (n == 0 || nprob == 0) { memset(out, 0, nprob * 64); *done = true; }
    return MINA_OK;
}

// ... and what they do alike: refuse scalars the digit recoding cannot take, upload them, run `msm(d_scalars, d_out_words)`, download nprob 17-word records, convert to bytes
template <class Msm>
static int host_msm_run(mina_ctx *c, size_t n, size_t nprob, const uint8_t *scalars, uint8_t *out, Msm &&msm) {
    if (!scalars_below_2_255(scalars, n * nprob)) return fail(MINA_ERR_ARG, "scalar >= 2^255");
    HIPC(hipSetDevice(c->device));
    c->use_lane0();
    MsmWorkspace &w = c->L->ws;
    if (int rc = w.out_words.ensure(nprob * 17 * 4)) return rc;
    if (int rc = h2d(c, w.scalars, scalars, nprob * n * 32)) return rc;
    if (int rc = msm(w.scalars.as<uint32_t>(), w.out_words.as<uint32_t>())) return rc;
    std::vector<uint32_t> hw(nprob * 17);
    if (int rc = d2h_sync(c, hw.data(), w.out_words, hw.size() * 4)) return rc;
    for (size_t m = 0; m < nprob; ++m) {
        if (hw[m * 17 + 16]) memset(out + m * 64, 0, 64);
        else memcpy(out + m * 64, &hw[m * 17], 64);
    }
    return MINA_OK;
}

extern "C" int mina_msm(mina_ctx *c, int curve, size_t n, const uint8_t *bases, const uint8_t *scalars, uint8_t *out) {
    bool done;
    if (int rc = host_msm_enter(c, curve, n, 1, bases && scalars, out, &done); rc || done) return rc;
    if (n > (1u << 24)) return fail(MINA_ERR_ARG, "n too large");
    return host_msm_run(c, n, 1, scalars, out, [&](const uint32_t *d_scalars, uint32_t *d_words) {
        if (int rc = h2d(c, c->L->tmp_a, bases, n * 64)) return rc;
        if (int rc = bases_to_mont(c, curve, n, c->L->tmp_a.p)) return rc;
        return mb_msm_variable(c, curve, (uint32_t)n, d_scalars, c->L->ws.points.p, d_words, nullptr);
    });
}

extern "C" int mina_msm_srs_range(mina_ctx *c, int curve, uint32_t first, size_t n, const uint8_t *scalars, uint8_t *out) {
    bool done;
    if (int rc = host_msm_enter(c, curve, n, 1, scalars != nullptr, out, &done); rc || done) return rc;
    if (n > 0xffffffffu) return fail(MINA_ERR_ARG, "n too large");
    return host_msm_run(c, n, 1, scalars, out, [&](const uint32_t *d_scalars, uint32_t *d_words) { return mb_msm_fixed(c, curve, (uint32_t)n, d_scalars, d_words, nullptr, first); });
}

extern "C" int mina_msm_srs(mina_ctx *c, int curve, size_t n, const uint8_t *scalars, uint8_t *out) { return mina_msm_srs_range(c, curve, 0, n, scalars, out); }

extern "C" int mina_msm_srs_multi(mina_ctx *c, int curve, size_t n, size_t nprob, const uint8_t *scalars, uint8_t *out) {
    bool done;
    if (int rc = host_msm_enter(c, curve, n, nprob, scalars != nullptr, out, &done); rc || done) return rc;
    SrsState &s = c->srs[curve];
    if (s.depth == 0) return fail(MINA_ERR_STATE, "SRS not loaded for this curve");
    if (n > s.depth || nprob > 4096) return fail(MINA_ERR_ARG, "n / nprob out of range");
    return host_msm_run(c, n, nprob, scalars, out, [&](const uint32_t *d_scalars, uint32_t *d_words) {
        return mb_msm_table(c, curve, s.table.p, s.depth, s.c, s.W, 0, (uint32_t)n, (uint32_t)nprob, d_scalars, d_words, nullptr);
    });
}
