#pragma once
// Fixed pool of host workers shared by the CalOccluded tasks of the step in phase A and the stateful tails of the step in phase B (sind_pipe, pipeline_impl.hpp).
// The GPU boxes give a process a bounded CPU share (16 cores per GPU on this pool): one bounded pool instead of a thread set per
// phase keeps the runnable threads under that share, which matters most in the pipelined mode where both kinds of task coexist.
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>
#include <pthread.h>
#include "common.hpp"

struct TaskGroup { std::mutex m; std::condition_variable cv; int left = 0; };
class WorkerPool {
public:
    void start(int n, int device, SindHostGate* gate, int spin_us = 0) {
        for (int i = 0; i < n; i++) th.emplace_back([this, i, device, gate, spin_us] {
            (void)pthread_setname_np(pthread_self(), "sind-worker");      // names show up in /proc/<pid>/task/*/comm (bench.py --thread-cpu)
            (void)hipSetDevice(device);
            t_sind_spin_us = spin_us;
            for (;;) {
                std::pair<std::function<void(int)>, TaskGroup*> job;
                { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [this] { return stop || !q.empty(); }); if (q.empty()) return; job = std::move(q.front()); q.pop_front(); }
                gate->acquire(); t_sind_gate = gate;          // a CPU token while the task computes (handed back inside every wait for the GPU)
                job.first(i);
                t_sind_gate = nullptr; gate->release();
                { std::lock_guard<std::mutex> lk(job.second->m); if (--job.second->left == 0) job.second->cv.notify_all(); }
            } });
    }
    void push(TaskGroup& g, std::function<void(int)> fn) {
        { std::lock_guard<std::mutex> lk(g.m); g.left++; }
        { std::lock_guard<std::mutex> lk(m); q.emplace_back(std::move(fn), &g); }
        cv.notify_one();
    }
    static void wait(TaskGroup& g) { std::unique_lock<std::mutex> lk(g.m); g.cv.wait(lk, [&g] { return g.left == 0; }); }
    int size() const { return (int)th.size(); }
    ~WorkerPool() { { std::lock_guard<std::mutex> lk(m); stop = true; } cv.notify_all(); for (auto& t : th) if (t.joinable()) t.join(); }
private:
    std::vector<std::thread> th; std::mutex m; std::condition_variable cv; std::deque<std::pair<std::function<void(int)>, TaskGroup*>> q; bool stop = false;
};
// a task that polls the GPU before it sleeps in a wait (common.hpp: t_sind_spin_us) for as long as this object lives: chains on an otherwise idle host
struct SpinScope { int keep; explicit SpinScope(bool on) : keep(t_sind_spin_us) { if (on) t_sind_spin_us = 400; } ~SpinScope() { t_sind_spin_us = keep; } };
