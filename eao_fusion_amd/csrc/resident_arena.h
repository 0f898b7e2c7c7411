// resident_arena.h -- the storage policy of the device-resident stores that outlive a call (eao_keyframe_db, eao_plane_map), free of HIP: the host's table
// of what an arena holds and the two capacity rules.  The device half is dev_arena.h; the walk programs under tools/ build this header alone.
//
// One arena of elements (words, points), appended to and never written in place.  An entry is a run begin .. begin + count - 1; a replaced or erased run stays
// in the arena as DEAD elements, which `used` still counts.  When the dead elements exceed HALF of the elements in use -- or nothing is live while entries
// remain -- the live runs are copied together, in table order, into a fresh allocation (plan_compaction: runs that follow one another in the old arena are ONE
// move, and a run that stays where it is is listed too, since the copies go into a fresh allocation), so an arena never holds more than twice its live elements
// plus its growth slack.  The table keeps ADD order: replace moves an entry's run to the end of the arena but not the entry's place.  Capacities are
// initial * 2^k: growth doubles until the need is covered, compaction leaves the smallest such capacity >= 2 * live, both clamped to the arena's maximum.
// The device work comes first and is all-or-nothing (dev_arena.h); the table changes -- append, replace, apply_compaction -- only after it has ended, so a
// failed call leaves table and arena as they were, and elements past `used` are never read.
#pragma once
#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <vector>

namespace eao {
namespace arena {

constexpr uint64_t kUnbounded = ~0ull;

// growth: the present capacity (or the initial one) doubled until it holds `need`
inline uint64_t grown_capacity(uint64_t cap, uint64_t initial, uint64_t need, uint64_t maxCap) {
    uint64_t c = cap ? cap : initial;
    while (c < need && c < maxCap) c *= 2;
    return c > maxCap ? maxCap : c;
}
// after a compaction: the smallest initial * 2^k that is at least twice the live elements
inline uint64_t compacted_capacity(uint64_t initial, uint64_t live, uint64_t maxCap) { return grown_capacity(0, initial, live * 2, maxCap); }

struct Move {      // compaction: count elements from src of the old arena to dst of the new one
    uint64_t src, dst, count;
};

struct NoPayload {};

template <typename Payload>
struct Entry : Payload {      // one run of the arena and what its owner keeps with it
    uint64_t id;
    uint64_t begin;
    uint32_t count;
    bool live;
};

template <typename Payload>
struct Table {
    std::vector<Entry<Payload>> entries;            // add order
    std::unordered_map<uint64_t, size_t> byId;      // live ids -> position in entries
    uint64_t used = 0, dead = 0;                    // elements of the arena in use (the dead ones included) / dead
    int32_t nLive = 0;

    void clear() {
        entries.clear();
        byId.clear();
        used = dead = 0;
        nLive = 0;
    }
    const Entry<Payload>* find(uint64_t id) const {
        auto it = byId.find(id);
        return it == byId.end() ? nullptr : &entries[it->second];
    }
    // appends; returns the arena position of the run's first element
    uint64_t append(uint64_t id, uint32_t n, const Payload& payload = Payload()) {
        Entry<Payload> e;
        static_cast<Payload&>(e) = payload;
        e.id = id;
        e.begin = used;
        e.count = n;
        e.live = true;
        byId[id] = entries.size();
        entries.push_back(e);
        used += n;
        nLive++;
        return e.begin;
    }
    // the old run dies where it lies, the new one goes to the end of the arena; the entry keeps its place in the table
    uint64_t replace(uint64_t id, uint32_t n) {
        Entry<Payload>& e = entries[byId.at(id)];
        dead += e.count;
        e.begin = used;
        e.count = n;
        used += n;
        return e.begin;
    }
    bool erase(uint64_t id) {
        auto it = byId.find(id);
        if (it == byId.end()) return false;
        Entry<Payload>& e = entries[it->second];
        e.live = false;
        dead += e.count;
        byId.erase(it);
        nLive--;
        return true;
    }
    bool wants_compaction() const { return dead * 2 > used || (nLive == 0 && !entries.empty()); }
    // the copies that bring the live runs together in table order; returns the live elements.  Nothing changes before apply_compaction().
    uint64_t plan_compaction(std::vector<Move>& moves) const {
        moves.clear();
        uint64_t at = 0;
        for (const Entry<Payload>& e : entries) {
            if (!e.live || e.count == 0) continue;
            if (!moves.empty() && moves.back().src + moves.back().count == e.begin) moves.back().count += e.count;
            else moves.push_back(Move{e.begin, at, e.count});
            at += e.count;
        }
        return at;
    }
    // drops the dead entries and closes the gaps
    void apply_compaction() {
        std::vector<Entry<Payload>> kept;
        kept.reserve((size_t)nLive);
        uint64_t at = 0;
        for (const Entry<Payload>& e : entries) {
            if (!e.live) continue;
            kept.push_back(e);
            kept.back().begin = at;
            at += e.count;
        }
        entries.swap(kept);
        byId.clear();
        for (size_t i = 0; i < entries.size(); i++) byId[entries[i].id] = i;
        used = at;
        dead = 0;
    }
};

}  // namespace arena
}  // namespace eao
