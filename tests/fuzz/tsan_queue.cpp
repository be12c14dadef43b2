// tsan_queue.cpp -- the race / stress tier of the boundary's completion queue (mina_verify_queue_*, include/mina_verify.h; the code sits at the end of
// mina_bridge_amd/csrc/api_verify.hip).  Built like tsan_boundary: the product's own host sources against the stand-in runtime of hip_stub/, the device layer
// stubbed -- by tsan_boundary.cpp itself, included below with its `main` renamed, so both tiers run on ONE stub and its answers:
//     * a state proof whose `ft_eval1` starts with "BAD!" fails its job's folded check (the boundary's fallback then finds exactly that proof): verdict 0;
//     * a state proof whose protocol states are cut short is rejected by the host parser: verdict 0;  every other fixture proof: verdict 1;
//     * an account pair whose public input starts with 0xBD: verdict 0, every other: 1.
// tests/test_verify_queue_host.py builds and runs it twice:
//   tsan_queue STATE.json ACCOUNT.json SECONDS   (-fsanitize=thread)  3 submitters (mixed kinds, random MINA_SUBMIT_MORE, now and then a flush), a consumer on
//       `wait`, a consumer on `poll` + the descriptor, 4 synchronous callers and a thread flipping merge / max_jobs / linger_us, all at once.  Afterwards: every
//       accepted tag completed exactly once with the stub's verdict, MINA_ERR_FULL was seen and only when `capacity` slots could have been held, a destroy with
//       entries in flight returned, nothing is left allocated.  Exit 0 = all of that and no race report (ThreadSanitizer exits with 66).
//   tsan_queue STATE.json ACCOUNT.json script    (-fsanitize=address,undefined)  a fixed script from one thread: the exact slot count behind MINA_ERR_FULL, buffers
//       freed right after `submit`, zero lengths, the descriptor's level, `wait`'s timeout, argument errors, destroy with pending entries, shutdown on an idle queue.
#define main tsan_boundary_main
#include "tsan_boundary.cpp"
#undef main

#include <poll.h>
#include <unistd.h>

namespace {
struct Fixtures { std::vector<std::string> proofs, pubs, bad_proofs, aproofs, apubs, bad_apubs; std::string truncated; };
struct Item { uint32_t kind; const std::string *proof, *pub; uint8_t want; };

bool load(const char *state_json, const char *account_json, Fixtures &f) {
    const std::string st = slurp(state_json), ac = slurp(account_json);
    for (auto &h : json_strings(st, "proof")) f.proofs.push_back(unhex(h));
    for (auto &h : json_strings(st, "pub")) f.pubs.push_back(unhex(h));
    { auto p = json_strings(ac, "proof"), q = json_strings(ac, "pub"); for (size_t i = 0; i < p.size() && i < 32; ++i) { f.aproofs.push_back(unb64(p[i])); f.apubs.push_back(unb64(q[i])); } }
    if (f.proofs.size() < 4 || f.proofs.size() != f.pubs.size() || f.aproofs.empty()) return false;
    for (auto &p : f.proofs) {                       // the failing variant of every state proof, as tsan_boundary makes it
        mw::StateProofContainer *box = new mw::StateProofContainer();
        mw::Bincode cur((const uint8_t *)p.data(), p.size());
        const bool ok = mw::read_wrap_proof(cur, box->tip_proof);
        const std::string needle((const char *)box->tip_proof.ft_eval1.b, 32);
        delete box;
        const size_t at = ok ? p.find(needle) : std::string::npos;
        if (at == std::string::npos || p.find(needle, at + 1) != std::string::npos) return false;
        std::string b = p; memcpy(&b[at], "BAD!", 4); f.bad_proofs.push_back(b);
    }
    for (auto &q : f.apubs) { std::string b = q; b[0] = (char)0xBD; f.bad_apubs.push_back(b); }
    f.truncated = f.proofs[0].substr(0, f.proofs[0].size() - 3000);
    return true;
}
// the r-th pair of a pseudo-random stream and the verdict the stub gives it
Item pick(const Fixtures &f, uint32_t r) {
    const uint32_t v = r >> 4;
    if (r & 1) { const size_t k = v % f.aproofs.size(); const bool bad = (r & 14) == 2; return Item{MINA_QUEUE_ACCOUNT, &f.aproofs[k], bad ? &f.bad_apubs[k] : &f.apubs[k], (uint8_t)!bad}; }
    const size_t k = v % f.proofs.size();
    if ((r & 14) == 2) return Item{MINA_QUEUE_STATE, &f.bad_proofs[k], &f.pubs[k], 0};
    if ((r & 14) == 4) return Item{MINA_QUEUE_STATE, &f.truncated, &f.pubs[0], 0};
    return Item{MINA_QUEUE_STATE, &f.proofs[k], &f.pubs[k], 1};
}
int submit(mina_verify_queue *q, const Item &it, uint64_t tag, uint32_t flags) {
    return mina_verify_queue_submit(q, it.kind, (const uint8_t *)it.proof->data(), it.proof->size(), (const uint8_t *)it.pub->data(), it.pub->size(), tag, flags);
}
bool install_index() {
    mina_verifier_index ix; memset(&ix, 0, sizeof ix); ix.log2_domain = 15; ix.zk_rows = 3;
    return mina_verify_install_verifier_index(&ix) == MINA_OK;
}
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

// ------------------------------------------------------------------------------------------------ the fixed script (AddressSanitizer / UBSan build)
int run_script(const Fixtures &f) {
    mina_verify_queue *q = nullptr; mina_verify_completion c[8]; size_t n = 99; uint64_t s[4];
    auto stats = [&](mina_verify_queue *qq) { return mina_verify_queue_stats(qq, &s[0], &s[1], &s[2], &s[3]); };
    // arguments
    q = (mina_verify_queue *)1; CHECK(mina_verify_queue_create(0, 1, &q) == MINA_ERR_ARG && !q);
    CHECK(mina_verify_queue_create(65537, 1, &q) == MINA_ERR_ARG && mina_verify_queue_create(4, 0, &q) == MINA_ERR_ARG && mina_verify_queue_create(4, 5, &q) == MINA_ERR_ARG && mina_verify_queue_create(4, 1, nullptr) == MINA_ERR_ARG);
    mina_verify_queue_destroy(nullptr);
    CHECK(mina_verify_queue_create(4, 1, &q) == MINA_OK && q);
    const Item good = Item{MINA_QUEUE_STATE, &f.proofs[0], &f.pubs[0], 1};
    const uint8_t *gp = (const uint8_t *)good.proof->data(), *gq = (const uint8_t *)good.pub->data();
    CHECK(mina_verify_queue_submit(q, 2, gp, 4, gq, 4, 0, 0) == MINA_ERR_ARG && mina_verify_queue_submit(q, 0, nullptr, 4, gq, 4, 0, 0) == MINA_ERR_ARG && mina_verify_queue_submit(q, 1, gp, 4, nullptr, 4, 0, 0) == MINA_ERR_ARG);
    CHECK(mina_verify_queue_submit(q, 0, gp, (1u << 20) + 1, gq, 4, 0, 0) == MINA_ERR_ARG && mina_verify_queue_submit(q, 0, gp, 4, gq, 4, 0, 2) == MINA_ERR_ARG && mina_verify_queue_submit(nullptr, 0, gp, 4, gq, 4, 0, 0) == MINA_ERR_ARG);
    CHECK(mina_verify_queue_poll(q, nullptr, 1, &n) == MINA_ERR_ARG && mina_verify_queue_poll(q, c, 8, nullptr) == MINA_ERR_ARG && mina_verify_queue_wait(nullptr, c, 8, &n, 0) == MINA_ERR_ARG);
    CHECK(mina_verify_queue_fd(nullptr) == MINA_ERR_ARG && mina_verify_queue_flush(nullptr) == MINA_ERR_ARG && stats(nullptr) == MINA_ERR_ARG);
    CHECK(stats(q) == MINA_OK && s[0] == 0 && s[1] == 0 && s[2] == 0 && s[3] == 0);
    // `wait` on an empty queue: nothing, after at least the timeout
    { const auto t0 = std::chrono::steady_clock::now(); CHECK(mina_verify_queue_wait(q, c, 8, &n, 20000) == MINA_OK && n == 0); CHECK(std::chrono::steady_clock::now() - t0 >= std::chrono::microseconds(20000)); }
    // slots: held from submit until the completion is handed out; buffers freed right after submit
    const int fd = mina_verify_queue_fd(q); CHECK(fd >= 0);
    struct pollfd pf = {fd, POLLIN, 0};
    for (uint64_t t = 0; t < 4; ++t) {
        const Item it = pick(f, (uint32_t)(16 * t + (t == 3 ? 2 : 0)));              // three good state proofs and a "BAD!" one
        uint8_t *hp = (uint8_t *)malloc(it.proof->size()), *hq = (uint8_t *)malloc(it.pub->size());
        memcpy(hp, it.proof->data(), it.proof->size()); memcpy(hq, it.pub->data(), it.pub->size());
        CHECK(mina_verify_queue_submit(q, it.kind, hp, it.proof->size(), hq, it.pub->size(), (t << 1) | it.want, MINA_SUBMIT_MORE) == MINA_OK);
        memset(hp, 0, it.proof->size()); free(hp); free(hq);
    }
    CHECK(submit(q, good, 99, 0) == MINA_ERR_FULL && stats(q) == MINA_OK && s[0] == 4 && s[1] == 0 && s[2] == 0);          // nothing has run
    CHECK(poll(&pf, 1, 0) == 0);
    CHECK(mina_verify_queue_flush(q) == MINA_OK);
    CHECK(poll(&pf, 1, 60000) == 1);                                               // one group, one write: all four are published
    CHECK(stats(q) == MINA_OK && s[1] == 4 && s[2] == 1 && s[3] == 4);
    CHECK(submit(q, good, 99, 0) == MINA_ERR_FULL);                                // ... and every slot is still held
    CHECK(mina_verify_queue_wait(q, c, 1, &n, -1) == MINA_OK && n == 1 && c[0].verdict == (c[0].tag & 1) && c[0].rc == MINA_OK && c[0].kind == MINA_QUEUE_STATE);
    CHECK(submit(q, good, (4u << 1) | 1, 0) == MINA_OK && submit(q, good, 99, 0) == MINA_ERR_FULL);
    { uint64_t seen = 1ull << (c[0].tag >> 1); size_t got = 1;
      while (got < 5) { CHECK(mina_verify_queue_wait(q, c, 8, &n, 60000000) == MINA_OK && n > 0); for (size_t i = 0; i < n; ++i, ++got) { CHECK(c[i].verdict == (c[i].tag & 1) && c[i].rc == MINA_OK && !(seen >> (c[i].tag >> 1) & 1)); seen |= 1ull << (c[i].tag >> 1); } }
      CHECK(seen == 31); }
    // the descriptor: cleared by the consumer, or by the poll that hands out the last completion
    CHECK(mina_verify_queue_poll(q, c, 8, &n) == MINA_OK && n == 0 && poll(&pf, 1, 0) == 0);
    CHECK(submit(q, pick(f, 1 + 16), 1, 0) == MINA_OK && poll(&pf, 1, 60000) == 1);
    { uint64_t v = 0; CHECK(read(fd, &v, 8) == 8 && v >= 1); }
    CHECK(mina_verify_queue_poll(q, c, 8, &n) == MINA_OK && n == 1 && c[0].verdict == 1 && c[0].kind == MINA_QUEUE_ACCOUNT && poll(&pf, 1, 0) == 0);
    CHECK(submit(q, pick(f, 1 + 2), 0, 0) == MINA_OK && poll(&pf, 1, 60000) == 1);
    CHECK(mina_verify_queue_poll(q, c, 8, &n) == MINA_OK && n == 1 && c[0].verdict == 0 && c[0].rc == MINA_OK && poll(&pf, 1, 0) == 0);
    // zero lengths are legal: the synchronous call's answer (`false` for a state proof)
    CHECK(mina_verify_queue_submit(q, MINA_QUEUE_STATE, nullptr, 0, nullptr, 0, 7, MINA_SUBMIT_MORE) == MINA_OK && mina_verify_queue_submit(q, MINA_QUEUE_ACCOUNT, nullptr, 0, gq, 0, 8, 0) == MINA_OK);
    const uint8_t empty[2] = {(uint8_t)mina_verify_state(gq, 0, gq, 0), (uint8_t)mina_verify_account(gq, 0, gq, 0)};      // (the stub's account job never reads a pair)
    CHECK(empty[0] == 0);
    for (size_t got = 0; got < 2; got += n) { CHECK(mina_verify_queue_wait(q, c, 8, &n, 60000000) == MINA_OK && n > 0); for (size_t i = 0; i < n; ++i) CHECK(c[i].kind == c[i].tag - 7 && c[i].verdict == empty[c[i].kind] && c[i].rc == MINA_OK); }
    // shutdown on an idle queue: usable afterwards (the contexts come back with the next job; the index is installed again as after any shutdown)
    CHECK(stats(q) == MINA_OK && s[0] == s[1]);
    mina_verify_shutdown();
    CHECK(mb_stub_live_allocs() == 0);
    CHECK(install_index() && submit(q, good, 1, 0) == MINA_OK && submit(q, pick(f, 4), 0, 0) == MINA_OK);
    for (size_t got = 0; got < 2; got += n) { CHECK(mina_verify_queue_wait(q, c, 8, &n, 60000000) == MINA_OK && n > 0); for (size_t i = 0; i < n; ++i) CHECK(c[i].verdict == c[i].tag && c[i].rc == MINA_OK); }
    // destroy with entries never flushed, and with completions never taken
    for (uint64_t t = 0; t < 3; ++t) CHECK(submit(q, pick(f, (uint32_t)(16 * t + (t & 1))), t, MINA_SUBMIT_MORE) == MINA_OK);
    mina_verify_queue_destroy(q);
    CHECK(mina_verify_queue_create(2, 4, &q) == MINA_OK && submit(q, good, 1, 0) == MINA_OK);
    mina_verify_queue_destroy(q);
    mina_verify_shutdown();
    CHECK(mb_stub_live_allocs() == 0);
    printf("{\"script\": \"ok\"}\n");
    return 0;
}

// ------------------------------------------------------------------------------------------------ the stress run (ThreadSanitizer build)
constexpr uint32_t CAPACITY = 64;
constexpr size_t MAX_SEQ = 1u << 22;
int run_stress(const Fixtures &f, double seconds) {
    mina_verify_queue *q = nullptr;
    CHECK(mina_verify_queue_create(CAPACITY, 2, &q) == MINA_OK);
    std::vector<std::atomic<uint8_t>> accepted(MAX_SEQ), seen(MAX_SEQ);
    for (size_t i = 0; i < MAX_SEQ; ++i) { accepted[i].store(0, std::memory_order_relaxed); seen[i].store(0, std::memory_order_relaxed); }
    std::atomic<bool> stop_submit{false}, stop_consume{false}, stop_rest{false};
    std::atomic<uint64_t> next_seq{0}, started{0}, rejected{0}, taken{0}, n_accepted{0}, full_seen{0}, full_wrong{0}, wrong{0}, sync_calls{0}, flushes{0};
    // tag = seq << 2 | kind << 1 | the verdict the stub gives
    auto submitter = [&](int id) {
        std::mt19937 rng(7 + id);
        while (!stop_submit.load()) {
            const uint64_t seq = next_seq.fetch_add(1);
            if (seq >= MAX_SEQ) break;
            const uint32_t r = rng(); const Item it = pick(f, r);
            const uint64_t taken_before = taken.load();                            // <= completions handed out when `submit` looks at the slots
            started.fetch_add(1);
            accepted[seq].store(1);                                                // (before the call: its completion may be taken before `submit` is back)
            const int rc = submit(q, it, seq << 2 | (uint64_t)it.kind << 1 | it.want, (r >> 20 & 1) ? MINA_SUBMIT_MORE : 0);
            if (rc == MINA_OK) n_accepted.fetch_add(1); else accepted[seq].store(0);
            if (rc == MINA_OK) {}
            else if (rc == MINA_ERR_FULL) {
                // full only with CAPACITY slots held: submissions accepted by then (at most: started - rejected, read afterwards) less completions handed out by
                // then (at least: `taken_before`) cannot be fewer
                const uint64_t rej = rejected.fetch_add(1) + 1, hi = started.load() - rej;
                full_seen.fetch_add(1);
                if (hi - taken_before < CAPACITY) full_wrong.fetch_add(1);
                (void)mina_verify_queue_flush(q); flushes.fetch_add(1);             // (what is held back by MINA_SUBMIT_MORE may be all there is)
                std::this_thread::yield();
            } else { wrong.fetch_add(1); fprintf(stderr, "submit: %d (%s)\n", rc, mina_last_error()); }
            if ((r >> 21 & 63) == 0) { (void)mina_verify_queue_flush(q); flushes.fetch_add(1); }
        }
    };
    auto account = [&](const mina_verify_completion *c, size_t n) {
        for (size_t i = 0; i < n; ++i) {
            const uint64_t seq = c[i].tag >> 2;
            if (seq >= MAX_SEQ || !accepted[seq].load() || c[i].rc != MINA_OK || c[i].verdict != (c[i].tag & 1) || c[i].kind != (c[i].tag >> 1 & 1)) {
                if (wrong.fetch_add(1) < 5) fprintf(stderr, "completion tag %llu: verdict %d rc %d kind %d\n", (unsigned long long)c[i].tag, c[i].verdict, c[i].rc, c[i].kind);
                continue;
            }
            seen[seq].fetch_add(1);
        }
        taken.fetch_add(n);
    };
    auto waiter = [&]() { mina_verify_completion c[16]; size_t n; while (!stop_consume.load()) { if (mina_verify_queue_wait(q, c, 16, &n, 5000) != MINA_OK) { wrong.fetch_add(1); break; } account(c, n); } };
    auto poller = [&]() {
        mina_verify_completion c[16]; size_t n; struct pollfd pf = {mina_verify_queue_fd(q), POLLIN, 0};
        while (!stop_consume.load()) {
            if (poll(&pf, 1, 5) <= 0) continue;
            uint64_t v; (void)!read(pf.fd, &v, 8);
            do { if (mina_verify_queue_poll(q, c, 16, &n) != MINA_OK) { wrong.fetch_add(1); return; } account(c, n); } while (n);
        }
    };
    auto sync_caller = [&](int id) {
        std::mt19937 rng(500 + id);
        while (!stop_rest.load()) {
            Item it = pick(f, (rng() & ~1u) | (uint32_t)(id & 1));
            const bool v = it.kind == MINA_QUEUE_STATE ? mina_verify_state((const uint8_t *)it.proof->data(), it.proof->size(), (const uint8_t *)it.pub->data(), it.pub->size())
                                                       : mina_verify_account((const uint8_t *)it.proof->data(), it.proof->size(), (const uint8_t *)it.pub->data(), it.pub->size());
            if (v != (it.want == 1)) wrong.fetch_add(1);
            sync_calls.fetch_add(1);
        }
    };
    auto tuner = [&]() {
        for (long it = 0; !stop_rest.load(); ++it) {
            std::this_thread::sleep_for(std::chrono::milliseconds(15));
            mina_verify_tuning t; mina_verify_tuning_get(&t);
            t.merge = (it % 5) ? 1 : 0; t.max_jobs = (it & 2) ? 2 : 1; t.linger_us = (it & 4) ? 0 : ((it & 1) ? 200 : 500);
            (void)mina_verify_configure_ex(&t);
        }
    };
    std::vector<std::thread> subs, cons, rest;
    for (int i = 0; i < 3; ++i) subs.emplace_back(submitter, i);
    cons.emplace_back(waiter); cons.emplace_back(poller);
    for (int i = 0; i < 4; ++i) rest.emplace_back(sync_caller, i);
    rest.emplace_back(tuner);
    std::this_thread::sleep_for(std::chrono::milliseconds((long)(seconds * 1000)));
    stop_submit.store(true);
    for (auto &t : subs) t.join();
    (void)mina_verify_queue_flush(q);
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(120);
    while (taken.load() < n_accepted.load() && std::chrono::steady_clock::now() < deadline) std::this_thread::sleep_for(std::chrono::milliseconds(2));
    stop_consume.store(true);
    for (auto &t : cons) t.join();
    uint64_t st[4]; CHECK(mina_verify_queue_stats(q, &st[0], &st[1], &st[2], &st[3]) == MINA_OK);
    // a second queue, destroyed with entries in flight (held back, dispatchable and running) while the synchronous callers are still at it
    mina_verify_queue *q2 = nullptr; CHECK(mina_verify_queue_create(256, 2, &q2) == MINA_OK);
    for (uint32_t i = 0; i < 200; ++i) CHECK(submit(q2, pick(f, i * 2654435761u), i, (i % 3) ? MINA_SUBMIT_MORE : 0) == MINA_OK);
    mina_verify_queue_destroy(q2);
    stop_rest.store(true);
    for (auto &t : rest) t.join();
    mina_verify_queue_destroy(q);
    mina_verify_configure_ex(nullptr);
    mina_verify_shutdown();
    uint64_t missing = 0, twice = 0, stray = 0;
    const uint64_t used = std::min<uint64_t>(next_seq.load(), MAX_SEQ);
    for (uint64_t i = 0; i < used; ++i) { const unsigned a = accepted[i].load(), s = seen[i].load(); if (a && s == 0) ++missing; if (s > 1) ++twice; if (!a && s) ++stray; }
    printf("{\"seconds\": %.1f, \"accepted\": %llu, \"taken\": %llu, \"full\": %llu, \"full_with_free_slots\": %llu, \"flushes\": %llu, \"jobs\": %llu, \"max_job\": %llu, \"sync_calls\": %llu, "
           "\"device_jobs\": %ld, \"culprit_searches\": %ld, \"account_jobs\": %ld, \"missing\": %llu, \"twice\": %llu, \"stray\": %llu, \"wrong\": %llu, \"live_allocs\": %ld}\n",
           seconds, (unsigned long long)n_accepted.load(), (unsigned long long)taken.load(), (unsigned long long)full_seen.load(), (unsigned long long)full_wrong.load(), (unsigned long long)flushes.load(),
           (unsigned long long)st[2], (unsigned long long)st[3], (unsigned long long)sync_calls.load(), g_jobs.load(), g_searches.load(), g_account_jobs.load(),
           (unsigned long long)missing, (unsigned long long)twice, (unsigned long long)stray, (unsigned long long)wrong.load(), mb_stub_live_allocs());
    CHECK(st[0] == n_accepted.load() && st[1] == st[0] && taken.load() == n_accepted.load());
    CHECK(n_accepted.load() > 0 && missing == 0 && twice == 0 && stray == 0 && wrong.load() == 0);
    CHECK(full_seen.load() > 0 && full_wrong.load() == 0);
    CHECK(st[2] > 0 && st[3] > 1 && st[3] <= CAPACITY && g_searches.load() > 0 && g_account_jobs.load() > 0 && sync_calls.load() > 0);
    CHECK(mb_stub_live_allocs() == 0);
    return 0;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s state_proofs_k15_bytes.json account_proofs_bytes.json seconds|script\n", argv[0]); return 2; }
    setenv("MINA_VERIFY_DEVICES", "0,0", 1);
    setenv("MINA_HOST_THREADS", "4", 1);
    Fixtures f;
    if (!load(argv[1], argv[2], f)) { fprintf(stderr, "fixtures not readable\n"); return 2; }
    mina_verify_configure(MINA_VERIFY_ALLOW_SURROGATE | MINA_VERIFY_ALLOW_UNBOUND_STATEMENT);   // as tsan_boundary: the kimchi step on the wrap index alone
    if (!install_index()) { fprintf(stderr, "install: %s\n", mina_last_error()); return 2; }
    return !strcmp(argv[3], "script") ? run_script(f) : run_stress(f, atof(argv[3]));
}
