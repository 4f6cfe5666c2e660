// pipe_trace.hpp -- the host pipeline's timeline instrument (lab builds;
// tools/pipe_trace.py).
#pragma once

#ifdef MXEC_LAB
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "runtime.hpp"

namespace mxec {

// MXEC_PIPE_TRACE=1 (lab builds): where a host reconstruct wave's time goes
// -- timing events on the copy and compute streams and host clocks around
// every wait, one stderr JSON line per wave (tools: the GET-stall study).
// The marks of every traced wave are reported against one process-wide
// reference event (recorded and completed by the first traced wave) and the
// host clock against one reference instant, so concurrent calls' traces line
// up.
struct PipeTrace {
    bool on = false;
    std::chrono::steady_clock::time_point h0;
    hipEvent_t e0 = nullptr;
    std::vector<std::pair<std::string, hipEvent_t>> ev;
    std::vector<std::pair<std::string, double>> host;
    static hipEvent_t& ref() {
        static hipEvent_t r = nullptr;
        return r;
    }
    static std::chrono::steady_clock::time_point& href() {
        static std::chrono::steady_clock::time_point t{};
        return t;
    }
    void start(hipStream_t s) {
        const char* e = getenv("MXEC_PIPE_TRACE");
        on = e && *e == '1';
        if (!on) return;
        static std::mutex mu;
        {
            std::lock_guard<std::mutex> g(mu);
            if (!ref()) {
                hipStream_t rs = nullptr;
                (void)hipStreamCreateWithFlags(&rs, hipStreamNonBlocking);
                (void)hipEventCreate(&ref());
                (void)hipEventRecord(ref(), rs);
                (void)hipEventSynchronize(ref());
                href() = std::chrono::steady_clock::now();
            }
        }
        h0 = href();
        e0 = ref();
        mark("start", s);
        now("start");
    }
    void mark(const char* what, hipStream_t s) {
        if (!on) return;
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        (void)hipEventRecord(e, s);
        ev.emplace_back(what, e);
    }
    void now(const char* what) {
        if (!on) return;
        host.emplace_back(what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count());
    }
    void report(const char* tag) {
        if (!on) return;
        now("end");
        std::string out = std::string("{\"pipe_trace\": \"") + tag + "\", \"gpu_ms\": [";
        for (size_t i = 0; i < ev.size(); ++i) {
            float ms = -1;
            (void)hipEventSynchronize(ev[i].second);
            (void)hipEventElapsedTime(&ms, e0, ev[i].second);
            char b[96];
            snprintf(b, sizeof b, "%s[\"%s\", %.3f]", i ? ", " : "", ev[i].first.c_str(), ms);
            out += b;
            (void)hipEventDestroy(ev[i].second);
        }
        out += "], \"host_ms\": [";
        for (size_t i = 0; i < host.size(); ++i) {
            char b[96];
            snprintf(b, sizeof b, "%s[\"%s\", %.3f]", i ? ", " : "", host[i].first.c_str(), host[i].second);
            out += b;
        }
        out += "]}";
        fprintf(stderr, "%s\n", out.c_str());
        ev.clear();
        host.clear();
    }
};

}  // namespace mxec
// In a class with a trace() accessor (HostCopy owns the call's PipeTrace).
#define PTRACE(x) trace().x
#else
#define PTRACE(x) ((void)0)
#endif
