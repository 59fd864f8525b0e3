// CPU sanitizer harness for the coalescing of concurrent ak_index_hybrid_search calls (archi_amd/csrc/coalesce.h: CoalescerT over
// HybridReq) -- TEST INFRASTRUCTURE. Built twice by archi_amd/csrc/Makefile -- `make tsan-hybrid` (-fsanitize=thread) and
// `make asan-hybrid` (-fsanitize=address,undefined) -- and run by tests/test_lexical_batch_cpu.py as a child process. The device
// side is a stand-in: run_group() plays lexical_batch.hip's lex_hybrid_group (one batch call per group).
//   phase 1, deterministic: while a first call is being served, 12 calls with ONE key and one call for every way a key can differ
//     (k, k1, b, sign, w_s, w_b -- one of them by a single bit --, filter pointer, length, epoch) queue up; when the first call
//     ends they are one batch: the 12 equal ones must be served by ONE group, every other one alone;
//   phase 2, 32 threads: random keys, requests and their output buffers on the caller's frame / heap of the caller's iteration
//     (freed as soon as submit() returns: a leader that touched a request after its owner left is a use-after-free under ASan and
//     a race under TSan, and the in-flight flags below catch it without a sanitizer); every request must be served exactly once,
//     with its OWN rows and an info that describes its group; k == 7 makes the group's call fail: every member gets the code and
//     the group's message, no other group does.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <set>
#include <thread>

#include "../../archi_amd/csrc/coalesce.h"

using namespace ak;

namespace {
constexpr int DIM = 4, ERR_FAKE = -7, MAX_OWNERS = 64;

struct FakeIndex {
    HybridCoalescer co;
    std::atomic<long> served{0}, launches{0}, largest{0};
    std::atomic<int> in_flight[MAX_OWNERS];          // 1 while owner t is inside submit(): its request may be touched
    std::atomic<int> hold{0};                        // phase 1: the first call waits here until the others have queued
    std::mutex log_mu;
    std::vector<std::vector<int>> groups;            // phase 1: the owners of every group served
    FakeIndex() { for (auto &f : in_flight) f = 0; }
};

bool bits_equal(double a, double b) { return !memcmp(&a, &b, 8); }
int owner_of(const HybridReq &r) { return (int)r.q[1]; }
int64_t expect_id(const float *q, int j) { return (int64_t)q[0] * 100 + j; }
double expect_comb(const HybridReq &r, int j) { return r.w_s * (double)j + r.w_b; }

void die(const char *what) { fprintf(stderr, "%s\n", what); abort(); }

// lex_hybrid_group's stand-in: one "batch call" for the group, every member's own rows written to the member's own buffers
void run_group(FakeIndex &ix, std::vector<HybridReq *> &g, bool log) {
    ix.launches++;
    if ((long)g.size() > ix.largest) ix.largest = (long)g.size();
    const HybridReq &h = *g[0];
    std::set<int64_t> also;
    std::vector<int> owners;
    for (auto *r : g) {
        // the grouping key, field by field (not through same_group): nothing that differs in any of them may share a call
        if (r->k != h.k || !bits_equal(r->k1, h.k1) || !bits_equal(r->b, h.b) || !bits_equal(r->sign, h.sign) || !bits_equal(r->w_s, h.w_s) ||
            !bits_equal(r->w_b, h.w_b) || r->filter != h.filter || r->flen != h.flen || r->fepoch != h.fepoch) die("group mixes keys");
        if (r->done) die("request served twice");
        if (!ix.in_flight[owner_of(*r)].load()) die("request outlived its owner's frame");
        for (int64_t i = 0; i < r->n_also; i++) also.insert(r->also[i]);
        owners.push_back(owner_of(*r));
    }
    if (log) {
        std::lock_guard<std::mutex> lk(ix.log_mu);
        ix.groups.push_back(owners);
    }
    while (ix.hold.load()) std::this_thread::yield();
    std::this_thread::sleep_for(std::chrono::microseconds(100 + (int)g.size() * 5));
    const int rc = h.k == 7 ? ERR_FAKE : 0;
    for (auto *r : g) {
        r->rc = rc;
        if (rc) { r->err = "fake failure of the call led by owner " + std::to_string(owner_of(h)); continue; }
        for (int j = 0; j < r->k; j++) {
            r->out_hit_ids[j] = expect_id(r->q, j);
            r->out_hit_comb[j] = expect_comb(*r, j);
            r->out_scan_ids[j] = -expect_id(r->q, j);
            r->out_scan_dist[j] = (double)r->T;
        }
        *r->n_hit = r->k; *r->n_scan = r->k - 1;
        if (r->out_info) { r->out_info[3] = (int64_t)also.size(); r->out_info[10] = g.size() > 1 ? (int64_t)g.size() : 0; }
    }
    ix.served += (long)g.size();
}

struct Call {                     // one caller's frame: the request, its inputs and its outputs
    std::vector<float> q; std::vector<int32_t> terms; std::vector<int64_t> also;
    std::vector<int64_t> hi, si; std::vector<double> hc, sd; int nh = -1, ns = -1; int64_t info[12];
    HybridReq req;
    Call(int owner, int serial, int k, double k1, double b, double sign, double w_s, double w_b, const uint8_t *f, int64_t flen, uint64_t fep,
         int T, int n_also)
        : q(DIM, 0.f), terms((size_t)T, 3), also((size_t)n_also), hi((size_t)k, -1), si((size_t)k, -1), hc((size_t)k, -1.0), sd((size_t)k, -1.0),
          req{q.data(), terms.data(), T, k1, b, sign, w_s, w_b, also.data(), n_also, f, flen, fep, k,
              hi.data(), hc.data(), &nh, si.data(), sd.data(), &ns, info} {
        q[0] = (float)serial; q[1] = (float)owner;
        for (int i = 0; i < n_also; i++) also[(size_t)i] = owner * 1000 + i;
        memset(info, 0, sizeof(info));
    }
    // what the owner must find after submit(): its own rows, or the failure of its group
    bool right(int rc) const {
        if (rc != req.rc) return false;
        if (req.k == 7) return rc == ERR_FAKE && req.err.rfind("fake failure of the call led by owner", 0) == 0;
        if (rc || nh != req.k || ns != req.k - 1 || info[3] < req.n_also) return false;
        for (int j = 0; j < req.k; j++)
            if (hi[(size_t)j] != expect_id(q.data(), j) || hc[(size_t)j] != expect_comb(req, j) || si[(size_t)j] != -expect_id(q.data(), j) ||
                sd[(size_t)j] != (double)req.T) return false;
        return true;
    }
};

int submit(FakeIndex *ix, Call &c, int owner, bool log) {
    ix->in_flight[owner] = 1;
    const int rc = ix->co.submit(c.req, [&](std::vector<HybridReq *> &g) { run_group(*ix, g, log); });
    ix->in_flight[owner] = 0;
    return rc;
}

// phase 1: what is served together and what is not
int grouping_phase() {
    auto ix = std::make_unique<FakeIndex>();
    static const uint8_t mask_a[16] = {1}, mask_b[16] = {1};
    const double w_b = 0.3, w_b_next = std::nextafter(0.3, 1.0);              // one bit apart: another key
    struct Key { int k; double k1, b, sign, w_s, w_b; const uint8_t *f; int64_t flen; uint64_t fep; };
    const Key base{5, 1.2, 0.75, 1.0, 0.7, w_b, mask_a, 16, 3};
    std::vector<Key> keys(12, base);                                          // owners 1..12: equal
    Key d;
    d = base; d.k = 6; keys.push_back(d);
    d = base; d.k1 = 1.5; keys.push_back(d);
    d = base; d.b = 0.5; keys.push_back(d);
    d = base; d.sign = -1.0; keys.push_back(d);
    d = base; d.w_s = 0.5; keys.push_back(d);
    d = base; d.w_b = w_b_next; keys.push_back(d);
    d = base; d.f = mask_b; keys.push_back(d);
    d = base; d.flen = 15; keys.push_back(d);
    d = base; d.fep = 4; keys.push_back(d);                                   // owners 13..21: each differs in one field
    std::atomic<int> bad{0};
    ix->hold = 1;
    std::thread first([&] {
        Call c(0, 0, 5, 1.2, 0.75, 1.0, 0.7, w_b, mask_a, 16, 3, 2, 0);
        if (!c.right(submit(ix.get(), c, 0, true))) bad++;
    });
    for (;;) {          // the first call is the leader and inside its group
        std::lock_guard<std::mutex> lk(ix->log_mu);
        if (!ix->groups.empty()) break;
    }
    std::vector<std::thread> ts;
    for (size_t i = 0; i < keys.size(); i++)
        ts.emplace_back([&, i] {
            const Key &x = keys[i];
            Call c((int)i + 1, (int)i + 1, x.k, x.k1, x.b, x.sign, x.w_s, x.w_b, x.f, x.flen, x.fep, 1 + (int)i % 3, (int)i % 4);
            if (!c.right(submit(ix.get(), c, (int)i + 1, true))) bad++;
            if (i < 12 && c.info[10] != 12) bad++;                            // the info of an equal one describes the shared call
            if (i >= 12 && c.info[10] != 0) bad++;
        });
    for (;;) {          // all of them queued behind the first call
        std::lock_guard<std::mutex> lk(ix->co.mu);
        if (ix->co.pending.size() == keys.size()) break;
    }
    ix->hold = 0;
    first.join();
    for (auto &t : ts) t.join();
    if (bad.load()) { fprintf(stderr, "FAILED: grouping phase, %d wrong answers\n", bad.load()); return 1; }
    // groups: {0}, the twelve equal ones together, nine groups of one
    size_t twelve = 0, ones = 0;
    for (auto &g : ix->groups) {
        if (g.size() == 12) { twelve++; for (int o : g) if (o < 1 || o > 12) return fprintf(stderr, "FAILED: a stranger in the equal group\n"), 1; }
        else if (g.size() == 1) ones++;
        else return fprintf(stderr, "FAILED: a group of %zu\n", g.size()), 1;
    }
    if (twelve != 1 || ones != 10 || ix->served != 22 || ix->co.busy || !ix->co.pending.empty())
        return fprintf(stderr, "FAILED: %zu groups of 12, %zu of 1, %ld served\n", twelve, ones, ix->served.load()), 1;
    return 0;
}

void caller(FakeIndex *ix, int tid, int iters, std::atomic<int> *bad) {
    std::mt19937 rng(4321 + tid);
    static const uint8_t masks[2][8] = {{1}, {1}};
    for (int it = 0; it < iters; it++) {
        const int k = (int[]){3, 5, 7}[rng() % 3], which = (int)(rng() % 3);
        const double w_s = (double[]){0.7, 0.5}[rng() % 2], w_b = (double[]){0.3, std::nextafter(0.3, 1.0)}[rng() % 2];
        const double sign = rng() % 2 ? 1.0 : -1.0;
        // the call's frame ends with the iteration: buffers freed, request gone
        auto c = std::make_unique<Call>(tid, tid * 100000 + it, k, 1.2, 0.75, sign, w_s, w_b, which < 2 ? masks[which] : nullptr,
                                        which < 2 ? 8 : 0, which < 2 ? 1 + rng() % 2 : 0, (int)(rng() % 5), (int)(rng() % 3));
        if (!c->right(submit(ix, *c, tid, false))) (*bad)++;
    }
}
}  // namespace

int main(int argc, char **argv) {
    const int threads = argc > 1 ? atoi(argv[1]) : 32, iters = argc > 2 ? atoi(argv[2]) : 100, bursts = argc > 3 ? atoi(argv[3]) : 2;
    if (threads > MAX_OWNERS) return fprintf(stderr, "at most %d threads\n", MAX_OWNERS), 2;
    if (grouping_phase()) return 1;
    long served = 0, launches = 0, largest = 0;
    for (int b = 0; b < bursts; b++) {
        auto *ix = new FakeIndex();
        std::atomic<int> bad{0};
        std::vector<std::thread> ts;
        for (int t = 0; t < threads; t++) ts.emplace_back(caller, ix, t, iters, &bad);
        for (auto &t : ts) t.join();
        if (bad.load() || ix->served != (long)threads * iters || ix->co.busy || !ix->co.pending.empty()) {
            fprintf(stderr, "FAILED: %d bad answers, %ld served of %ld, busy=%d, pending=%zu\n", bad.load(), ix->served.load(), (long)threads * iters,
                    (int)ix->co.busy, ix->co.pending.size());
            delete ix;
            return 1;
        }
        served += ix->served; launches += ix->launches; largest = std::max(largest, ix->largest.load());
        delete ix;                                                      // destroy while idle
    }
    printf("ok: grouping pinned (12 equal calls in one group, 9 differing ones alone); %ld requests in %ld group calls (largest %ld), "
           "%d bursts x %d threads\n", served, launches, largest, bursts, threads);
    return 0;
}
