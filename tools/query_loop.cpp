// The host loop over matchy_query that whole-line mode replaces, as a program of its own (tools/time_whole_lines.py builds and runs
// it): opens DATABASE, reads QUERIES (one per line), and answers all of them on THREADS host threads (contiguous shares), REPS
// times. Prints one JSON line: queries, found, seconds of the fastest repetition, queries per second.
//   g++ -O2 -std=c++17 tools/query_loop.cpp -Iinclude -Lmatchy_amd/lib -lmatchy_amd -lpthread -Wl,-rpath,$PWD/matchy_amd/lib -o query_loop
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <thread>
#include <vector>

#include "matchy_amd.h"

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: query_loop DATABASE QUERIES THREADS [REPS]\n"); return 2; }
    const int threads = std::max(1, atoi(argv[3])), reps = argc > 4 ? std::max(1, atoi(argv[4])) : 3;
    matchy_t* db = matchy_open(argv[1]);
    if (!db) { fprintf(stderr, "cannot open %s: %s\n", argv[1], matchy_amd_last_error()); return 1; }
    std::vector<std::string> qs;
    {
        std::ifstream f(argv[2], std::ios::binary);
        std::string line;
        while (std::getline(f, line)) qs.push_back(line);
    }
    double best = 1e30;
    unsigned long long found_all = 0;
    for (int r = 0; r < reps; ++r) {
        std::atomic<unsigned long long> found{0};
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; ++t)
            pool.emplace_back([&, t] {
                const size_t lo = qs.size() * (size_t)t / (size_t)threads, hi = qs.size() * (size_t)(t + 1) / (size_t)threads;
                unsigned long long n = 0;
                for (size_t i = lo; i < hi; ++i) {
                    matchy_result_t res = matchy_query(db, qs[i].c_str());
                    n += res.found ? 1 : 0;
                    matchy_free_result(&res);
                }
                found += n;
            });
        for (auto& th : pool) th.join();
        best = std::min(best, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        found_all = found;
    }
    printf("{\"threads\": %d, \"queries\": %zu, \"found\": %llu, \"seconds\": %.6f, \"queries_per_s\": %.0f}\n", threads, qs.size(), found_all, best,
           best > 0 ? (double)qs.size() / best : 0.0);
    matchy_close(db);
    return 0;
}
