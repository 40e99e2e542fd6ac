// Host side: the hipGraph replay cache of a model handle (lsl_sample / lsl_sample_ex).  A call whose arguments (pointers, sizes, step
// table: the key) repeat is captured once and replayed; the small-batch configs are launch-bound (~700 launches of a few microseconds per
// sampling call).  The first appearance of a key runs eagerly (it also initialises the per-kernel attributes), the second is captured,
// later ones are replayed.  Included by host_common.hip.h in front of lsl_model.
#pragma once

struct GraphCache {
    struct Key : std::vector<unsigned char> {  // the bytes of everything a call's enqueued launches depend on
        void put(const void *p, size_t bytes) { insert(end(), (const unsigned char *)p, (const unsigned char *)p + bytes); }
        template <class T>
        void put(const T &value) { put(&value, sizeof(value)); }  // (a pointer: the pointer itself)
    };
    struct Entry {
        Key key;
        hipGraphExec_t exec = nullptr;
        unsigned long long last_use = 0;
    };
    std::vector<Entry> graphs;      // at most 8, least recently used evicted
    std::vector<Key> seen;          // keys that ran eagerly once (capture happens on their second appearance); the last 16
    std::vector<Key> uncapturable;  // keys whose capture failed: never tried again; the last 16
    bool stream_failed = false;     // the internal capture stream could not be created: no further attempts
    unsigned long long clock = 0;
    hipStream_t stream = nullptr;  // capture happens on this internal stream (the caller's may be the legacy default stream, which
                                   // cannot be captured); the instantiated graph is launched on the caller's stream

    void clear() {  // (captured launches hold the handle's weight pointers, pass size and forms: whatever changes those calls this)
        for (auto &g : graphs)
            if (g.exec) hipGraphExecDestroy(g.exec);
        graphs.clear();
        seen.clear();
        uncapturable.clear();
    }
    ~GraphCache() {
        clear();
        if (stream) hipStreamDestroy(stream);
    }

    // One call with this key on stream st; enqueue(stream) puts its launches on a stream and returns 0 or a fail() code.
    // Returns 1: the call is on st (replayed, or captured now and launched); 0: the caller runs it eagerly (first sighting recorded, or not
    // capturable); < 0: fail() code.
    template <class Enqueue>
    int run(const Key &key, hipStream_t st, Enqueue &&enqueue) {
        auto has = [&](const std::vector<Key> &v) { return std::find(v.begin(), v.end(), key) != v.end(); };
        auto launch = [&](hipGraphExec_t exec) { return hipGraphLaunch(exec, st) == hipSuccess ? 1 : fail(-10, "hipGraphLaunch failed"); };
        for (auto &g : graphs)
            if (g.key == key) {
                g.last_use = ++clock;
                return launch(g.exec);
            }
        if (stream_failed || has(uncapturable)) return 0;  // capture failed before for this key (or no capture stream): eager from now on
        if (!has(seen)) {
            if (seen.size() >= 16) seen.erase(seen.begin());
            seen.push_back(key);
            return 0;
        }
        hipGraph_t graph = nullptr;
        if (!stream && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) {
            stream = nullptr;
            stream_failed = true;
        }
        if (stream && hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            const int rc = enqueue(stream);
            const hipError_t e = hipStreamEndCapture(stream, &graph);
            hipGraphExec_t exec = nullptr;
            if (rc == 0 && e == hipSuccess && graph && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess) {
                hipGraphDestroy(graph);
                if (graphs.size() >= 8) {  // evict the least recently used
                    auto lru = std::min_element(graphs.begin(), graphs.end(), [](const Entry &a, const Entry &b) { return a.last_use < b.last_use; });
                    hipGraphExecDestroy(lru->exec);
                    graphs.erase(lru);
                }
                graphs.push_back(Entry{key, exec, ++clock});
                return launch(exec);
            }
            if (graph) hipGraphDestroy(graph);
        }
        (void)hipGetLastError();  // capture not possible: forget the error, run eagerly, and never try this key again
        seen.erase(std::find(seen.begin(), seen.end(), key));
        if (uncapturable.size() >= 16) uncapturable.erase(uncapturable.begin());
        uncapturable.push_back(key);
        return 0;
    }
};
