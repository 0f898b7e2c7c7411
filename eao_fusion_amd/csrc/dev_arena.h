// dev_arena.h -- the device half of resident_arena.h: one or more parallel columns of device memory that share a capacity (the word ids and values of
// eao_keyframe_db; the points of eao_plane_map).  Both operations build EVERY column anew and swap only once all of it has ended: on any failure the fresh
// blocks are freed and the old columns and the capacity stand.
#pragma once
#include <tuple>
#include <utility>
#include <vector>

#include "common.h"
#include "resident_arena.h"

namespace eao {

template <typename... Ts>
struct DevArena {
    std::tuple<Ts*...> col{};      // cap elements each
    size_t cap = 0;
    const size_t initial, maxCap;

    explicit DevArena(size_t initial_, uint64_t maxCap_ = arena::kUnbounded) : initial(initial_), maxCap((size_t)maxCap_) {}
    DevArena(const DevArena&) = delete;
    DevArena& operator=(const DevArena&) = delete;
    ~DevArena() { release(col); }

    template <size_t I = 0>
    auto at() const { return std::get<I>(col); }

    // room for `need` elements, the first `used` of every column kept
    eao_status reserve(uint64_t need, uint64_t used, hipStream_t stream) {
        if (need <= cap) return EAO_OK;
        std::vector<arena::Move> keep;
        if (used > 0) keep.push_back(arena::Move{0, 0, used});
        return rebuild(keep, (size_t)arena::grown_capacity(cap, initial, need, maxCap), stream);
    }
    size_t compacted_capacity(uint64_t live) const { return (size_t)arena::compacted_capacity(initial, live, maxCap); }
    // the moves of a planned compaction into columns of newCap; the caller applies the table's compaction only after EAO_OK
    eao_status compact(const std::vector<arena::Move>& moves, size_t newCap, hipStream_t stream) { return rebuild(moves, newCap, stream); }

private:
    static void release(const std::tuple<Ts*...>& c) {
        std::apply([](auto*... p) { ((void)(p ? hipFree(p) : hipSuccess), ...); }, c);
    }
    template <size_t... I>
    hipError_t fill(std::tuple<Ts*...>& fresh, const std::vector<arena::Move>& moves, size_t newCap, hipStream_t stream, std::index_sequence<I...>) {
        hipError_t e = hipSuccess;
        ((e = e != hipSuccess ? e : hipMalloc((void**)&std::get<I>(fresh), newCap * sizeof(Ts))), ...);
        for (size_t m = 0; m < moves.size(); m++)
            ((e = e != hipSuccess ? e : hipMemcpyAsync(std::get<I>(fresh) + moves[m].dst, std::get<I>(col) + moves[m].src, moves[m].count * sizeof(Ts),
                                                       hipMemcpyDeviceToDevice, stream)), ...);
        const hipError_t sync = hipStreamSynchronize(stream);      // (also after a failure: no copy is in flight when the fresh blocks are freed)
        return e != hipSuccess ? e : sync;
    }
    eao_status rebuild(const std::vector<arena::Move>& moves, size_t newCap, hipStream_t stream) {
        std::tuple<Ts*...> fresh{};
        const hipError_t e = fill(fresh, moves, newCap, stream, std::index_sequence_for<Ts...>());
        if (e != hipSuccess) {      // nothing changed: the old columns and the caller's table stand
            release(fresh);
            EAO_HIP(e);
        }
        release(col);
        col = fresh;
        cap = newCap;
        return EAO_OK;
    }
};

// The step that ends an erase and a replace: when the table wants it, the live runs into fresh columns (ctx: the calling thread's stream context).
template <typename Ctx, typename Table, typename... Ts>
eao_status compact_if_wanted(Ctx& ctx, Table& table, DevArena<Ts...>& dev) {
    if (!table.wants_compaction()) return EAO_OK;
    eao_status st = ctx.ready(StreamClass::Latency);
    if (st) return st;
    std::vector<arena::Move> moves;
    const uint64_t live = table.plan_compaction(moves);
    if ((st = dev.compact(moves, dev.compacted_capacity(live), ctx.stream))) return st;
    table.apply_compaction();
    return EAO_OK;
}

}  // namespace eao
