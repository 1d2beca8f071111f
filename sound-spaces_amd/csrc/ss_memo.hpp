// ss_memo.hpp — the reference's per-pose observation memo for the column path (pure host C++, no HIP:
// tests/pose_memo_host.cpp drives it on its own; ss_hip.hip, ss_ctx_observe_sims_memo, issues the launches it plans).
//
// The reference memoises observations per pose (soundspaces/simulator.py:678-701): the key is (source, receiver, azimuth)
// and ignores _audio_index, _audio_index advances inside a miss only (:634-635), and the caches are dropped when the scene
// or the sound changes (:395-397).  Here: per env a tag (scene, sound) and a map pose key -> row of a device-side pool the
// caller owns; one free list over the pool's rows.  A step is PLANNED first (nothing changes) and COMMITTED last:
//   * an env whose tag changed drops its map first - its rows return to the free list and may serve this very step;
//   * a key that is present is a HIT: the env is held (rendered as a silent unit, audio_index not advanced) and its output
//     row is fetched from the pool row;
//   * a key that is absent is a MISS: the env is rendered and its output row is stored into a free pool row - silent envs
//     too (the reference caches its zeros under the pose as well).
// A step that needs more rows than the pool has commits nothing; plan() says how many rows the pool needs in total.
// Row numbering is this file's own business.
#pragma once
#include <cstdint>
#include <unordered_map>
#include <vector>

namespace ssmemo {

// (source, receiver, azimuth), each field below 2^20 (ss_amd/vector.py: the same word the Python observer keys its maps with)
inline uint64_t pose_key(long long src, long long recv, long long azimuth) {
    return (static_cast<uint64_t>(src) << 40) | (static_cast<uint64_t>(recv) << 20) | static_cast<uint64_t>(azimuth);
}
inline long long azimuth_of(long long rot) {                       // simulator.py:573
    long long az = (-rot) % 360;
    return az < 0 ? az + 360 : az;
}

struct Env {
    bool tagged = false;
    long long scene = 0, sound = 0;
    std::unordered_map<uint64_t, int> rows;                        // pose key -> pool row
};

struct Memo {
    std::vector<Env> envs;
    std::vector<int> free_rows;                                    // stack: rows given back last are taken first
    int pool_rows = 0;                                             // rows the free list knows of (in use + free)
    int in_use = 0;
    long long hits = 0, misses = 0, dropped = 0;                   // dropped: maps dropped by a scene / sound change
    // the plan of the step (valid between plan() and commit())
    std::vector<unsigned char> hold, drop;
    std::vector<uint64_t> key;
    std::vector<int> hit_row;
    int plan_hits = 0, plan_misses = 0, plan_rows = -1;

    void reset(int n_envs) {
        envs.assign(static_cast<size_t>(n_envs), Env{});
        free_rows.clear();
        pool_rows = in_use = 0;
        hits = misses = dropped = 0;
        hold.assign(static_cast<size_t>(n_envs), 0);
        drop.assign(static_cast<size_t>(n_envs), 0);
        key.assign(static_cast<size_t>(n_envs), 0);
        hit_row.assign(static_cast<size_t>(n_envs), -1);
        plan_rows = -1;
    }
    void clear() { reset(static_cast<int>(envs.size())); }         // forget every pose, keep the size
    int n_envs() const { return static_cast<int>(envs.size()); }

    // Plan one step of n == n_envs() envs against a pool of `rows` rows.  Changes nothing but the plan.  Returns -1 for a bad
    // call (n, a pool smaller than the one rows were handed out of), 0 when the step fits (hold[i] says which envs are held;
    // commit() may follow), else the number of rows the pool needs in total (> rows; nothing to commit).
    int plan(const long long* scene, const long long* sound, const long long* src, const long long* recv, const long long* rot,
             int n, int rows) {
        plan_rows = -1;
        if (n != n_envs() || rows < pool_rows || !scene || !sound || !src || !recv || !rot) return -1;
        int freed = 0;
        plan_hits = plan_misses = 0;
        for (int i = 0; i < n; ++i) {
            const Env& e = envs[static_cast<size_t>(i)];
            drop[i] = !e.tagged || e.scene != scene[i] || e.sound != sound[i];
            key[i] = pose_key(src[i], recv[i], azimuth_of(rot[i]));
            hit_row[i] = -1;
            if (drop[i]) {
                freed += static_cast<int>(e.rows.size());
            } else {
                auto it = e.rows.find(key[i]);
                if (it != e.rows.end()) hit_row[i] = it->second;
            }
            hold[i] = hit_row[i] >= 0;
            plan_hits += hold[i];
            plan_misses += !hold[i];
        }
        const int need = in_use - freed + plan_misses;
        if (need > rows) return need;
        plan_rows = rows;
        return 0;
    }

    // Commit the step plan() accepted: drops, new entries, counters.  moves [n][2] = {env (= output row), pool row}: the step's
    // n_store misses first, then its n_fetch hits.  Envs are distinct and pool rows are distinct over the whole list.
    // scene / sound: the columns the step was planned from (the new tags of the envs whose maps were dropped).
    void commit(const long long* scene, const long long* sound, int* moves, int* n_store, int* n_fetch) {
        const int n = n_envs();
        *n_store = *n_fetch = 0;
        if (plan_rows < 0) return;
        for (int r = plan_rows - 1; r >= pool_rows; --r) free_rows.push_back(r);      // the pool has grown: lowest row first
        pool_rows = plan_rows;
        for (int i = 0; i < n; ++i) {
            if (!drop[i]) continue;
            Env& e = envs[static_cast<size_t>(i)];
            for (const auto& kv : e.rows) free_rows.push_back(kv.second);
            in_use -= static_cast<int>(e.rows.size());
            e.rows.clear();
            if (e.tagged) ++dropped;
            e.tagged = true; e.scene = scene[i]; e.sound = sound[i];
        }
        int k = 0;
        for (int i = 0; i < n; ++i) {
            if (hold[i]) continue;
            const int r = free_rows.back();
            free_rows.pop_back();
            ++in_use;
            envs[static_cast<size_t>(i)].rows.emplace(key[i], r);
            moves[2 * k] = i; moves[2 * k + 1] = r;
            ++k;
        }
        *n_store = k;
        for (int i = 0; i < n; ++i) {
            if (!hold[i]) continue;
            moves[2 * k] = i; moves[2 * k + 1] = hit_row[i];
            ++k;
        }
        *n_fetch = k - *n_store;
        hits += plan_hits;
        misses += plan_misses;
        plan_rows = -1;
    }
};

}  // namespace ssmemo
