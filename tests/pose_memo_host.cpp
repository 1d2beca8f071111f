// pose_memo_host.cpp — TEST INFRASTRUCTURE: the pose memo's bookkeeping (sound-spaces_amd/csrc/ss_memo.hpp) on its own, without
// HIP, against a model written from the reference's rule (soundspaces/simulator.py:678-701, :634-635, :395-397): per env a dict
// pose -> the observation first rendered there, dropped when the scene or the sound changes; a hit returns the cached
// observation and does not advance _audio_index.  An "observation" here is one integer naming what was rendered (0 = silence,
// else sound and clip window); the pool is an array of such integers and the moves the memo plans are carried out on it as
// k_memo_rows would carry them out - so the check is end to end (the right content reaches the right env) and never compares
// pool row numbers.  tests/test_pose_memo_host.py builds this with -fsanitize=address,undefined and runs it.
// Never part of the product.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "../sound-spaces_amd/csrc/ss_memo.hpp"

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                                                              \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::printf("FAIL %s:%d: %s | ", __FILE__, __LINE__, #cond);              \
            std::printf(__VA_ARGS__);                                                 \
            std::printf("\n");                                                        \
            if (++g_fail > 20) std::exit(1);                                          \
        }                                                                             \
    } while (0)

constexpr int kWindows = 3;                      // a 3-s sound: _audio_index runs 0, 1, 2, 0, ...

struct EnvState {                                // what a simulator holds (the columns of ss_sim_columns)
    long long scene = 0, sound = 0, src = 2, recv = 0, rot = 0, audio_index = 0, step_count = 0, duration = 1 << 30;
};

int content_of(const EnvState& e) { return e.step_count > e.duration ? 0 : 1 + static_cast<int>(e.sound) * 100 + static_cast<int>(e.audio_index); }
bool multi_second(const EnvState& e) { return e.sound != 1; }      // sound 1 is the 1-s sound: its window never moves

// the reference, per env
struct ModelEnv {
    bool tagged = false;
    long long scene = 0, sound = 0;
    std::map<uint64_t, int> cache;
    long long audio_index = 0;
};

struct World {
    int n;
    std::vector<EnvState> st;                    // driven by the walk; audio_index is the memo side's
    std::vector<ModelEnv> model;
    ssmemo::Memo memo;
    std::vector<int> pool;                       // pool row -> content
    int pool_rows;
    long long m_hits = 0, m_misses = 0, m_dropped = 0;
    int grows = 0;

    World(int n_envs, int rows) : n(n_envs), st(n_envs), model(n_envs), pool(rows, -1), pool_rows(rows) { memo.reset(n_envs); }

    // one step of all envs; returns the number of pool rows the step took without growing (for the reuse check)
    void step(int t, bool may_grow = true) {
        std::vector<long long> scene(n), sound(n), src(n), recv(n), rot(n);
        for (int i = 0; i < n; ++i) { scene[i] = st[i].scene; sound[i] = st[i].sound; src[i] = st[i].src; recv[i] = st[i].recv; rot[i] = st[i].rot; }
        // ---- the model
        std::vector<int> want(n);
        std::vector<char> m_hit(n);
        for (int i = 0; i < n; ++i) {
            ModelEnv& m = model[i];
            if (!m.tagged || m.scene != scene[i] || m.sound != sound[i]) {
                if (m.tagged) ++m_dropped;
                m.cache.clear(); m.tagged = true; m.scene = scene[i]; m.sound = sound[i];
            }
            const uint64_t key = ssmemo::pose_key(src[i], recv[i], ssmemo::azimuth_of(rot[i]));
            auto it = m.cache.find(key);
            m_hit[i] = it != m.cache.end();
            if (m_hit[i]) { want[i] = it->second; ++m_hits; continue; }
            ++m_misses;
            EnvState e = st[i];
            e.audio_index = m.audio_index;
            want[i] = content_of(e);
            if (want[i] != 0 && multi_second(e)) m.audio_index = (m.audio_index + 1) % kWindows;
            m.cache.emplace(key, want[i]);
        }
        size_t live = 0;
        for (const ModelEnv& m : model) live += m.cache.size();
        // ---- the memo: plan (grow and plan again when told to), render, commit, move
        const long long h0 = memo.hits, mi0 = memo.misses, d0 = memo.dropped;
        const int u0 = memo.in_use;
        int need = memo.plan(scene.data(), sound.data(), src.data(), recv.data(), rot.data(), n, pool_rows);
        CHECK(need >= 0, "step %d: plan refused", t);
        if (need > 0) {
            CHECK(need == static_cast<int>(live), "step %d: need_rows %d, the model holds %zu entries", t, need, live);
            CHECK(need > pool_rows, "step %d: need_rows %d with %d rows", t, need, pool_rows);
            CHECK(memo.hits == h0 && memo.misses == mi0 && memo.dropped == d0 && memo.in_use == u0, "step %d: a refused plan changed the counters", t);
            int ns = -1, nf = -1;
            std::vector<int> none(2 * n, -7);
            memo.commit(scene.data(), sound.data(), none.data(), &ns, &nf);          // nothing to commit: must be a no-op
            CHECK(ns == 0 && nf == 0 && memo.in_use == u0 && memo.hits == h0, "step %d: commit after a refused plan", t);
            CHECK(may_grow, "step %d: the pool had to grow to %d rows", t, need);
            pool.resize(need, -1);                                                // the caller grows the pool, contents kept
            pool_rows = need;
            ++grows;
            need = memo.plan(scene.data(), sound.data(), src.data(), recv.data(), rot.data(), n, pool_rows);
            CHECK(need == 0, "step %d: plan after growing says %d", t, need);
        }
        std::vector<int> out(n);
        for (int i = 0; i < n; ++i) {
            CHECK(!!memo.hold[i] == !!m_hit[i], "step %d env %d: held %d, the model says hit %d", t, i, memo.hold[i], m_hit[i]);
            if (memo.hold[i]) { out[i] = 0; continue; }                           // a silent unit; audio_index stays
            out[i] = content_of(st[i]);
            if (out[i] != 0 && multi_second(st[i])) st[i].audio_index = (st[i].audio_index + 1) % kWindows;
        }
        std::vector<int> moves(2 * n, -1);
        int n_store = 0, n_fetch = 0;
        memo.commit(scene.data(), sound.data(), moves.data(), &n_store, &n_fetch);
        CHECK(n_store + n_fetch == n, "step %d: %d stores + %d fetches for %d envs", t, n_store, n_fetch, n);
        std::set<int> rows, slots;
        for (int k = 0; k < n_store + n_fetch; ++k) {
            const int r = moves[2 * k], s = moves[2 * k + 1];
            CHECK(r >= 0 && r < n && s >= 0 && s < pool_rows, "step %d move %d: row %d slot %d", t, k, r, s);
            CHECK(rows.insert(r).second && slots.insert(s).second, "step %d move %d: row %d or slot %d named twice", t, k, r, s);
            CHECK((k < n_store) == !memo.hold[r], "step %d move %d: wrong half of the list", t, k);
        }
        for (int k = 0; k < n_store; ++k) pool[moves[2 * k + 1]] = out[moves[2 * k]];              // (order is free: distinct)
        for (int k = n_store; k < n_store + n_fetch; ++k) out[moves[2 * k]] = pool[moves[2 * k + 1]];
        for (int i = 0; i < n; ++i) {
            CHECK(out[i] == want[i], "step %d env %d: observation %d, the reference gives %d", t, i, out[i], want[i]);
            CHECK(st[i].audio_index == model[i].audio_index, "step %d env %d: audio_index %lld vs %lld", t, i, st[i].audio_index, model[i].audio_index);
        }
        CHECK(memo.in_use == static_cast<int>(live), "step %d: %d rows in use, the model holds %zu entries", t, memo.in_use, live);
        CHECK(memo.hits == m_hits && memo.misses == m_misses && memo.dropped == m_dropped, "step %d: counters %lld/%lld/%lld vs %lld/%lld/%lld", t,
              memo.hits, memo.misses, memo.dropped, m_hits, m_misses, m_dropped);
        CHECK(static_cast<int>(memo.free_rows.size()) + memo.in_use == memo.pool_rows && memo.pool_rows == pool_rows, "step %d: free list", t);
    }
};

// (receiver, rotation, step_count, sound) per step and env, duration 6: the script of tests/test_vector.py's pose-cache test
void scripted() {
    World w(2, 1);                               // one pool row: the first step already has to grow
    struct M { int recv, rot, cnt, snd; };
    const M script[][2] = {{{1, 90, 0, 0}, {2, 0, 0, 0}}, {{1, 90, 1, 0}, {2, 0, 1, 0}},       // stand still: hit, index frozen
                           {{3, 90, 2, 0}, {2, 90, 2, 0}}, {{1, 90, 3, 0}, {2, 0, 3, 0}},      // leave; come back: the FIRST window
                           {{4, 180, 4, 0}, {4, 0, 4, 0}}, {{4, 180, 7, 0}, {1, 0, 7, 0}},     // silence after the duration
                           {{1, 90, 8, 1}, {1, 0, 8, 0}},                                      // env 0 changes its sound
                           {{1, 90, 9, 1}, {2, 0, 9, 0}}};
    int t = 0;
    for (const auto& mv : script) {
        for (int i = 0; i < 2; ++i) {
            EnvState& e = w.st[i];
            if (e.sound != mv[i].snd) { e.sound = mv[i].snd; e.audio_index = 0; w.model[i].audio_index = 0; }
            e.recv = mv[i].recv; e.rot = mv[i].rot; e.step_count = mv[i].cnt; e.duration = 6;
        }
        w.step(t++);
    }
    CHECK(w.m_hits >= 5 && w.m_misses >= 8 && w.m_dropped == 1, "script: %lld hits %lld misses %lld drops", w.m_hits, w.m_misses, w.m_dropped);
    CHECK(w.grows >= 2, "script: the pool grew %d times", w.grows);
    // a scene change drops the map as a sound change does
    w.st[1].scene = 5;
    w.step(t++);
    CHECK(w.m_dropped == 2, "scene change: %lld drops", w.m_dropped);
}

// rows freed by a tag change serve the misses of the same step: the pool is full, env 0 drops 3 rows while both envs miss
void reuse_in_the_same_step() {
    World w(2, 6);
    for (int k = 0; k < 3; ++k) {                // 3 poses per env: 6 rows, the pool is full
        w.st[0].recv = k; w.st[1].recv = 10 + k;
        w.step(k, false);
    }
    CHECK(w.memo.in_use == 6 && w.memo.free_rows.empty(), "pool not full: %d in use", w.memo.in_use);
    std::set<int> freed;
    for (const auto& kv : w.memo.envs[0].rows) freed.insert(kv.second);
    w.st[0].sound = 2; w.st[0].audio_index = 0; w.model[0].audio_index = 0;        // env 0: new sound, its 3 rows are free again
    w.st[0].recv = 7; w.st[1].recv = 20;                                          // both envs miss: 2 rows needed, 0 free before
    w.step(3, false);                                                             // (may_grow = false: growing is a failure here)
    CHECK(w.pool_rows == 6 && w.memo.in_use == 5, "reuse: %d rows, %d in use", w.pool_rows, w.memo.in_use);
    for (int i = 0; i < 2; ++i)
        for (const auto& kv : w.memo.envs[i].rows)
            if ((i == 0) || kv.first == ssmemo::pose_key(2, 20, 0)) CHECK(freed.count(kv.second) == 1, "reuse: env %d took row %d", i, kv.second);
}

void bad_calls() {
    ssmemo::Memo m;
    m.reset(2);
    const long long z[2] = {0, 0};
    CHECK(m.plan(z, z, z, z, z, 3, 8) == -1, "n != n_envs accepted");
    CHECK(m.plan(z, z, z, z, nullptr, 2, 8) == -1, "a NULL column accepted");
    CHECK(m.plan(z, z, z, z, z, 2, 1) == 2, "two misses into one row");
    CHECK(m.plan(z, z, z, z, z, 2, 8) == 0, "plan");
    int mv[4], ns, nf;
    m.commit(z, z, mv, &ns, &nf);
    CHECK(ns == 2 && nf == 0 && m.pool_rows == 8, "commit");
    CHECK(m.plan(z, z, z, z, z, 2, 4) == -1, "a pool smaller than the one rows were handed out of accepted");
    CHECK(m.plan(z, z, z, z, z, 2, 8) == 0 && m.hold[0] && m.hold[1], "standing still is a hit");
    m.clear();
    CHECK(m.in_use == 0 && m.pool_rows == 0 && m.hits == 0 && m.n_envs() == 2, "clear");
    CHECK(m.plan(z, z, z, z, z, 2, 2) == 0 && !m.hold[0], "after clear every pose is new");
    // azimuth = -rot mod 360, in [0, 360)
    CHECK(ssmemo::azimuth_of(90) == 270 && ssmemo::azimuth_of(-90) == 90 && ssmemo::azimuth_of(0) == 0 && ssmemo::azimuth_of(450) == 270, "azimuth");
}

// seeded walk: 8 envs over 6 poses with 3-s and 1-s sounds, sound and scene changes, durations that run out; the pool starts at
// 2 rows and is grown to exactly what the memo asks for, every time
void random_walk(unsigned seed, int steps) {
    std::mt19937 rng(seed);
    auto uni = [&](int k) { return static_cast<int>(rng() % static_cast<unsigned>(k)); };
    World w(8, 2);
    for (int t = 0; t < steps; ++t) {
        for (int i = 0; i < w.n; ++i) {
            EnvState& e = w.st[i];
            const int r = uni(100);
            if (r < 40) { const int p = uni(6); e.recv = p % 3; e.rot = 90 * (p / 3) - 90; }        // one of 6 poses (else: stand still)
            ++e.step_count;
            if (r >= 92) {                                                                       // a new episode
                const long long snd = uni(3);
                if (snd != e.sound) { e.sound = snd; e.audio_index = 0; w.model[i].audio_index = 0; }
                if (r >= 97) e.scene = uni(2);
                e.step_count = 0; e.duration = 2 + uni(6);
            }
        }
        w.step(t);
    }
    CHECK(w.m_hits > steps && w.m_misses > steps && w.m_dropped > 5, "walk %u: %lld hits %lld misses %lld drops", seed, w.m_hits, w.m_misses, w.m_dropped);
    std::printf("walk seed %u: %d steps, %lld hits, %lld misses, %lld maps dropped, pool grown %d times to %d rows\n", seed, steps, w.m_hits,
                w.m_misses, w.m_dropped, w.grows, w.pool_rows);
}

}  // namespace

int main() {
    bad_calls();
    scripted();
    reuse_in_the_same_step();
    random_walk(1, 400);
    random_walk(2, 400);
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("pose memo: ok\n");
    return 0;
}
