// devbuf_unit.cpp -- who frees what: DevBuf / PinnedBuf (mina_bridge_amd/csrc/ctx.h) and the objects that hold them, against the stand-in runtime of hip_stub/,
// whose mb_stub_live_allocs() counts the blocks nobody has freed yet.  A stand-alone host program under AddressSanitizer and UBSan (`make -C tests/fuzz devbuf_unit`,
// then ./devbuf_unit; tests/test_devbuf_ownership.py): a block freed twice, or written after its free, is a sanitizer report; a block never freed is a count.
// Exit code 0 = every check held.
#include <cstdio>
#include <cstring>
#include <memory>

#include "../../mina_bridge_amd/csrc/ctx.h"

int mb_fail(int code, const std::string &msg) { fprintf(stderr, "mb_fail %d: %s\n", code, msg.c_str()); return code; }
mina_verify_tuning mb_tune() { mina_verify_tuning t; memset(&t, 0, sizeof t); return t; }

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { ++g_failed; fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)
static long live() { return mb_stub_live_allocs(); }

template <class Buf> static void ensure_grow_scope() {      // what DevBuf and PinnedBuf share
    {
        Buf b;
        CHECK(live() == 0 && b.p == nullptr && b.cap == 0);
        CHECK(b.ensure(100) == MINA_OK && b.p && b.cap >= 100 && live() == 1);            // an empty buffer allocates
        void *const p0 = b.p; const size_t cap0 = b.cap;
        CHECK(b.ensure(40) == MINA_OK && b.p == p0 && b.cap == cap0 && live() == 1);      // smaller: nothing happens
        CHECK(b.ensure(cap0 + 1) == MINA_OK && b.cap > cap0 && live() == 1);              // larger: the old block is gone, one is live
        memset(b.p, 0x5a, b.cap);
        b.release(); CHECK(b.p == nullptr && b.cap == 0 && live() == 0);
        b.release(); CHECK(live() == 0);                                                  // twice is harmless
        CHECK(b.ensure(64) == MINA_OK && live() == 1);
    }
    CHECK(live() == 0);                                                                   // the scope's end frees it
}

static void aliases() {
    DevBuf parent;
    CHECK(parent.ensure(1000) == MINA_OK && live() == 1);
    void *const pp = parent.p; const size_t pcap = parent.cap;
    {
        DevBuf view;
        view.alias(parent);
        CHECK(view.p == pp && view.cap == pcap && view.borrowed && live() == 1);          // the count does not change
        CHECK(view.ensure(pcap) == MINA_OK && view.p == pp && view.borrowed);             // within the parent's capacity: still the parent's block
    }
    CHECK(live() == 1 && parent.p == pp);                                                 // the view's end does not free the parent's block
    memset(parent.p, 0x11, parent.cap);                                                   // ... which is still writable
    {
        DevBuf view;
        view.alias(parent);
        CHECK(view.ensure(pcap + 1) == MINA_OK);                                          // outgrown: an allocation of its own
        CHECK(!view.borrowed && view.p != pp && view.cap > pcap && live() == 2);
        CHECK(parent.p == pp && parent.cap == pcap);
        memset(parent.p, 0x22, parent.cap); memset(view.p, 0x33, view.cap);
    }
    CHECK(live() == 1);                                                                   // the view's own block: freed once, with the view
    {
        DevBuf own;
        CHECK(own.ensure(10) == MINA_OK && live() == 2);
        own.alias(parent);                                                                // over an owned buffer: the owned block goes first
        CHECK(live() == 1 && own.p == pp && own.borrowed);
        DevBuf empty; own.alias(empty);                                                   // of an empty buffer: empty, and nothing borrowed
        CHECK(own.p == nullptr && own.cap == 0 && !own.borrowed && live() == 1);
    }
    memset(parent.p, 0x44, parent.cap);
    parent.release();
    CHECK(live() == 0);                                                                   // the parent's block: freed once, by the parent
}

static void whole_objects() {
    {
        Lane *l = new Lane();
        CHECK(l->ws.buckets29.ensure(300) == MINA_OK && l->gs_flags.ensure(8) == MINA_OK && l->host_stage.ensure(5000) == MINA_OK && live() == 3);
        delete l;
        CHECK(live() == 0);
    }
    {
        SrsState *s = new SrsState();
        CHECK(s->table.ensure(4096) == MINA_OK && s->lagrange_digits29.ensure(512) == MINA_OK && live() == 2);
        delete s;
        CHECK(live() == 0);
    }
    {
        mina_ctx *c = new mina_ctx();
        CHECK(c->dedup_totals.ensure(16) == MINA_OK && c->acct_defaults.ensure(3 * 32) == MINA_OK && c->pparams[1].ensure(2048) == MINA_OK && live() == 3);
        delete c;
        CHECK(live() == 0);
    }
}

static void views() {
    std::unique_ptr<mina_ctx> parent(new mina_ctx());
    Installed &p = *parent;
    CHECK(p.srs[0].table.ensure(4096) == MINA_OK && p.pparams[0].ensure(2048) == MINA_OK && p.state_salts.ensure(576) == MINA_OK && p.kimchi_index.ensure(700) == MINA_OK);
    p.srs[0].depth = 64; p.srs[0].srs_gen = 7; p.have_pparams[0] = true; p.have_state_salts = true; p.have_kimchi = true; p.kimchi_log2 = 15;
    const long owned = live();
    CHECK(owned == 4);
    Installed *v = new Installed();
    v->borrow_from(p);
    CHECK(live() == owned);                                                               // a view owns nothing
    CHECK(v->srs[0].table.p == p.srs[0].table.p && v->srs[0].table.cap == p.srs[0].table.cap && v->srs[0].table.borrowed && v->srs[0].depth == 64 && v->srs[0].srs_gen == 7);
    CHECK(v->pparams[0].p == p.pparams[0].p && v->pparams[0].cap == p.pparams[0].cap && v->have_pparams[0]);
    CHECK(v->state_salts.p == p.state_salts.p && v->state_salts.cap == p.state_salts.cap && v->have_state_salts);
    CHECK(v->kimchi_index.p == p.kimchi_index.p && v->kimchi_index.cap == p.kimchi_index.cap && v->have_kimchi && v->kimchi_log2 == 15);
    CHECK(v->srs[1].table.p == nullptr && !v->srs[1].table.borrowed && v->pparams[1].p == nullptr);      // nothing installed: nothing borrowed
    const size_t cap0 = p.srs[0].table.cap;
    CHECK(p.srs[0].table.ensure(cap0 + 1) == MINA_OK && live() == owned);                 // the parent installs a larger table: its old block is gone ...
    v->borrow_from(p);                                                                    // ... and the next refresh picks up the new one
    CHECK(v->srs[0].table.p == p.srs[0].table.p && v->srs[0].table.cap == p.srs[0].table.cap && v->srs[0].table.cap > cap0 && live() == owned);
    delete v;                                                                             // view before parent
    CHECK(live() == owned);
    memset(p.srs[0].table.p, 0x66, p.srs[0].table.cap); memset(p.kimchi_index.p, 0x66, p.kimchi_index.cap);
    parent.reset();
    CHECK(live() == 0);
}

int main() {
    ensure_grow_scope<DevBuf>();
    ensure_grow_scope<PinnedBuf>();
    aliases();
    whole_objects();
    views();
    if (g_failed || live()) { fprintf(stderr, "devbuf_unit: %d checks failed, %ld allocations still live\n", g_failed, live()); return 1; }
    return 0;
}
