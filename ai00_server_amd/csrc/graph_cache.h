// graph_cache.h — the policy for keeping captured step graphs, host-only (no HIP include; tests/test_graph_cache_cpp.py compiles it with g++).
//
// GraphCache<Key, Handle, Deleter> owns opaque handles (the engine's are hipGraphExec_t) under one policy:
//   * a key is captured the SECOND time it shows up: decode-shaped steps repeat at once, while the one-off shapes of prefill tails would pay
//     capture + instantiation (milliseconds) for a single replay and churn the cache.  The set of keys seen once is bounded: the insertion
//     that takes it past SEEN_MAX clears it of every key but the one just inserted (the others wait one more visit, nothing else);
//   * at most `capacity` handles are kept; a full cache gives up the one whose last find() / insert() is oldest, the rest stay warm;
//   * every handle goes through the deleter exactly once: at eviction, clear() or destruction.
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>
#include <set>

namespace rwkv {

template <class Key, class Handle, class Deleter>
class GraphCache {
public:
    static constexpr size_t SEEN_MAX = 4096;
    GraphCache(size_t capacity, Deleter del) : cap_(capacity), del_(del) {}
    GraphCache(const GraphCache &) = delete;
    GraphCache &operator=(const GraphCache &) = delete;
    ~GraphCache() { clear(); }

    // the cached handle (now the most recently used), or nullptr
    Handle *find(const Key &key) {
        auto it = entries_.find(key);
        if (it == entries_.end()) return nullptr;
        it->second.used = ++clock_;
        return &it->second.handle;
    }
    // for a key find() did not know: false on its first visit (run it directly), true from then on (capture it)
    bool should_capture(const Key &key) {
        if (!seen_.insert(key).second) return true;
        if (seen_.size() > SEEN_MAX) { seen_.clear(); seen_.insert(key); }
        return false;
    }
    // takes ownership of the handle of a key find() did not know; the reference holds until the next insert() / clear()
    Handle &insert(const Key &key, Handle handle) {
        if (entries_.size() >= cap_ && !entries_.empty()) {
            auto victim = entries_.begin();
            for (auto o = entries_.begin(); o != entries_.end(); ++o) if (o->second.used < victim->second.used) victim = o;
            del_(victim->second.handle);
            entries_.erase(victim);
        }
        return entries_.emplace(key, Entry{handle, ++clock_}).first->second.handle;
    }
    void clear() {
        for (auto &e : entries_) del_(e.second.handle);
        entries_.clear();
        seen_.clear();
    }

private:
    struct Entry { Handle handle; uint64_t used; };
    size_t cap_;
    Deleter del_;
    uint64_t clock_ = 0;
    std::map<Key, Entry> entries_;
    std::set<Key> seen_;
};

}  // namespace rwkv
