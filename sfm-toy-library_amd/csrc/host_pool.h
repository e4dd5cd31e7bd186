// host_pool.h -- the small thread pool of the image readers' host halves (jpeg_entropy.cpp, png_inflate.cpp): item(i) for every
// i in 0..n-1, one item at a time per thread, with at most min(n, max_threads, 16) threads (the caller's thread is one of them).
// Plain C++, header only, so that each host half still compiles alone under the sanitizers.  item must not throw.
#pragma once
#include <algorithm>
#include <atomic>
#include <system_error>
#include <thread>
#include <vector>

namespace sfmba {

template <typename Item> void host_pool_for(int n, int max_threads, Item item) {
    if (n <= 0) return;
    std::atomic<int> next(0);
    auto work = [&]() {
        for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) item(i);
    };
    const int n_threads = std::max(1, std::min(n, std::min(max_threads, 16)));
    std::vector<std::thread> pool;
    try {
        for (int t = 1; t < n_threads; ++t) pool.emplace_back(work);
    } catch (const std::system_error&) {                       // fewer threads than asked for: the rest of the work is done here
    }
    work();
    for (std::thread& t : pool) t.join();
}

}  // namespace sfmba
