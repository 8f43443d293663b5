// The set-up's worker threads: one pool (parallelFor), the draw-ahead loop that keeps a threaded pass on the
// sequential random stream (parallelDraws), and the same loop with the density sums taken on a device
// (deviceSampling).
#pragma once

#include <algorithm>
#include <atomic>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "mt_random.hpp"
#include "ski_parse.hpp"

#pragma GCC visibility push(hidden)  // the library's own: not among its dynamic symbols
namespace skirt {

// Runs fn(i0, i1) over [0, n) in ranges of at most `grain` items on min(16, hardware) worker threads, which take
// the ranges from one atomic cursor; the caller runs meanwhile() beside them and then waits. A worker's exception
// ends that worker; the first one (in worker order) is thrown on the caller as std::runtime_error with its message.
template <class Fn, class Meanwhile>
void parallelFor(size_t n, size_t grain, Fn fn, Meanwhile meanwhile) {
    const int T = std::max(1, std::min(16, (int)std::thread::hardware_concurrency()));
    std::atomic<size_t> next{0};
    std::vector<std::thread> th;
    std::vector<std::string> errs(T + 1);
    for (int w = 0; w < T; w++)
        th.emplace_back([&, w] {
            try {
                for (size_t i; (i = next.fetch_add(grain)) < n;) fn(i, std::min(n, i + grain));
            } catch (std::exception& ex) {
                errs[w] = ex.what();
            }
        });
    try {
        meanwhile();
    } catch (std::exception& ex) {
        errs[T] = ex.what();
    }
    for (auto& t : th) t.join();
    for (auto& e : errs)
        if (!e.empty()) throw std::runtime_error(e);
}
template <class Fn>
void parallelFor(size_t n, size_t grain, Fn fn) {
    parallelFor(n, grain, fn, [] {});
}

// Runs fn(q, u) for the items q in [0, n) on worker threads, where u points to the `per` uniform
// deviates item q would have drawn had the items been processed one after the other, drawing as they
// go: the deviates are drawn ahead, in item order, one chunk at a time (the next chunk while the
// workers evaluate the current one). Results are therefore identical to the sequential loop's.
template <class Fn>
void parallelDraws(UniformSource& rng, size_t n, int per, Fn fn) {
    if (n == 0) return;
    const size_t chunk = std::max<size_t>(1, (size_t)(1 << 20) / std::max(1, per));
    // the Mersenne twister hands over raw words (the sequential part); the workers convert them
    MTRandom* mt = dynamic_cast<MTRandom*>(&rng);
    std::vector<uint32_t> wbuf[2];
    std::vector<double> dbuf[2];
    auto draw = [&](int k, size_t q0) {
        const size_t m = (std::min(n, q0 + chunk) - q0) * per;
        if (mt) {
            wbuf[k].resize(m);
            mt->words(wbuf[k].data(), m);
        } else {
            dbuf[k].resize(m);
            for (double& u : dbuf[k]) u = rng.uniform();
        }
    };
    draw(0, 0);
    for (size_t q0 = 0, k = 0; q0 < n; q0 += chunk, k ^= 1) {
        const size_t q1 = std::min(n, q0 + chunk);
        parallelFor(
            q1 - q0, 64,
            [&](size_t e0, size_t e1) {
                std::vector<double> u(per);
                for (size_t e = e0; e < e1; e++) {
                    if (mt) {
                        const uint32_t* y = &wbuf[k][e * per];
                        for (int i = 0; i < per; i++) u[i] = MTRandom::deviate(y[i]);
                        fn(q0 + e, u.data());
                    } else {
                        fn(q0 + e, &dbuf[k][e * per]);
                    }
                }
            },
            [&] {
                if (q1 < n) draw((int)(k ^ 1), q1);
            });
    }
}

// The density sampling of n items on the sampler's device, when there is one and the setup stream is the
// Mersenne twister: item q gets the 3 * nsample words the sequential loop would draw for it, in item
// order; the items go in chunks, the next chunk's words drawn while the device samples the current one.
// box(q, b) fills item q's box, apply(q, out) takes its sums. False: no device sampling (nothing drawn).
template <class BoxFn, class ApplyFn>
bool deviceSampling(const Ctx& c, const std::vector<DustComp>& dust, size_t n, int nsample, int mode, BoxFn box,
                    ApplyFn apply) {
    MTRandom* mt = dynamic_cast<MTRandom*>(c.rng);
    if (!c.sampler || !mt || n == 0) return false;
    const size_t per = 3 * (size_t)nsample;
    const size_t chunk = std::max<size_t>(1, ((size_t)1 << 26) / per);  // 64 Mi words (256 MiB) per call
    const size_t nout = mode == kDensNode ? 6 : dust.size();
    std::vector<uint32_t> w[2];
    std::vector<double> boxes, out;
    auto draw = [&](int k, size_t q0) {
        w[k].resize((std::min(n, q0 + chunk) - q0) * per);
        mt->words(w[k].data(), w[k].size());
    };
    draw(0, 0);
    for (size_t q0 = 0, k = 0; q0 < n; q0 += chunk, k ^= 1) {
        const size_t q1 = std::min(n, q0 + chunk);
        std::thread next;
        if (q1 < n) next = std::thread(draw, (int)(k ^ 1), q1);
        try {
            boxes.resize(6 * (q1 - q0));
            for (size_t q = q0; q < q1; q++) box(q, &boxes[6 * (q - q0)]);
            out.resize(nout * (q1 - q0));
            c.sampler->sample(dust, boxes.data(), q1 - q0, w[k].data(), nsample, mode, out.data());
            for (size_t q = q0; q < q1; q++) apply(q, &out[nout * (q - q0)]);
        } catch (...) {
            if (next.joinable()) next.join();
            throw;
        }
        if (next.joinable()) next.join();
    }
    return true;
}

}  // namespace skirt
#pragma GCC visibility pop
