// Part of libnellie_hip.so: included by nellie_comm.hip (host code + one small kernel).
// =================================================================================================
// Loopback transport: the nccl* subset this library uses, between contexts of ONE process
// =================================================================================================
// Why: the Z-slab path exchanges ghost planes, bit planes, reductions and tables through RCCL, and a box with one GPU can
// only ever run that code with one rank -- where no send / recv is issued at all.  This transport implements the same calls
// (ncclSend / ncclRecv inside groups, ncclAllReduce, ncclAllGather, ncclBroadcast, group semantics, communicator set-up by
// unique id) between `world` contexts living in one process, one host thread per rank, with device-to-device copies ON THE
// STREAM THE CALLER PASSES.  Everything above the nccl* call -- which planes, which offsets and counts, which stream and
// communicator, the events that order the side stream against the compute stream, `halo_pending` -- runs unchanged, so the
// N >= 2 code paths execute on one GPU with exactly the arguments RCCL will see.
//
// Semantics kept: an operation is ENQUEUED on the caller's stream; data at the source is read in stream order of the
// sender (an event recorded on the sender's stream at the call), lands in stream order of the receiver, and the sender's
// stream does not run past the operation before the data has been read (an event recorded by the reader).  What differs
// from RCCL: the host threads rendezvous inside the call (RCCL's kernels rendezvous on the device), so every rank must make
// the same calls in the same order -- which the SPMD path does.
//
// NELLIE_LOOPBACK_DELAY_US=n: every transfer is preceded, on its stream, by a kernel spinning a pseudo-random 0..n us, so
// that a missing stream / event dependency in the code above shows as stale data instead of passing by luck.
#include <unistd.h>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <set>

namespace lb {

static const char kMagic[8] = {'N', 'L', 'L', 'O', 'O', 'P', 'B', 'K'};
enum { kMissing = 1000 };       // ncclResult_t value for "librccl.so could not be loaded" (see CommApi below)

struct Msg {
    const void *src = nullptr;
    size_t bytes = 0;
    hipEvent_t ready = nullptr, done = nullptr;
    bool consumed = false;
};

struct Group {
    std::string id;
    int world = 0, joined = 0, refs = 0;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    unsigned long long gen = 0;
    bool broken = false;                       // a rendezvous timed out: every later wait fails at once
    std::vector<int> device;                  // per rank: its HIP device (kernels of one rank read staging blocks of the others)
    std::vector<const void *> send;           // per rank: what the current collective reads
    std::vector<hipEvent_t> ev_ready, ev_done;
    std::vector<void *> staging;
    std::vector<size_t> staging_cap;
    std::vector<std::deque<Msg *>> chan;       // [src * world + dst]
};

struct Comm {
    Group *g = nullptr;
    int rank = 0;
    unsigned long long rng = 0;
};

struct Op {
    int kind;                                   // 0 send, 1 recv, 2 all-reduce, 3 all-gather, 4 broadcast
    const void *src; void *dst; size_t count; ncclDataType_t dt; ncclRedOp_t op; int peer; Comm *comm; hipStream_t st;
    Msg *msg = nullptr;
};

static std::mutex g_mu;
static std::map<std::string, Group *> g_groups;
static std::set<void *> g_comms;
static std::atomic<unsigned long long> g_ids{1};
static thread_local int t_depth = 0;
static thread_local std::vector<Op> t_ops;

static inline bool is_ours(const void *comm) {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_comms.count(const_cast<void *>(comm)) != 0;
}
static inline bool is_loopback_id(const char *id128) { return memcmp(id128, kMagic, 8) == 0; }

static int timeout_s() {
    static int v = 0;
    if (!v) { const char *e = getenv("NELLIE_LOOPBACK_TIMEOUT_S"); v = (e && atoi(e) > 0) ? atoi(e) : 120; }
    return v;
}
static int delay_us() {
    const char *e = getenv("NELLIE_LOOPBACK_DELAY_US");
    return (e && atoi(e) > 0) ? atoi(e) : 0;
}

static size_t dt_size(ncclDataType_t dt) {
    switch (dt) {
        case ncclChar: case ncclUint8: return 1;
        case ncclInt32: case ncclUint32: case ncclFloat: return 4;
        case ncclInt64: case ncclUint64: case ncclDouble: return 8;
        default: return 0;
    }
}

__global__ void spin_kernel(unsigned long long ticks) {
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
// pseudo-random delay in front of a transfer (see the header)
static void jitter(Comm *c, hipStream_t st) {
    const int mx = delay_us();
    if (!mx) return;
    c->rng = c->rng * 6364136223846793005ull + 1442695040888963407ull;
    const unsigned long long us = (c->rng >> 33) % (unsigned long long)(mx + 1);
    if (us) spin_kernel<<<1, 1, 0, st>>>(us * 100ull);      // wall_clock64 ticks at 100 MHz
}

struct Ptrs { const void *p[16]; };
template <typename T>
__global__ void reduce_kernel(Ptrs src, int world, T *dst, size_t n, int op) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    T acc = ((const T *)src.p[0])[i];
    for (int r = 1; r < world; ++r) {
        const T v = ((const T *)src.p[r])[i];
        acc = op == 0 ? (T)(acc + v) : (op == 1 ? (v < acc ? v : acc) : (v > acc ? v : acc));
    }
    dst[i] = acc;
}

// every rank of the group passes here before any leaves; false: timed out (a rank died or the ranks disagree on the calls)
static bool barrier(Group *g, std::unique_lock<std::mutex> &lk) {
    if (g->broken) return false;
    const unsigned long long my = g->gen;
    if (++g->arrived == g->world) { g->arrived = 0; ++g->gen; g->cv.notify_all(); return true; }
    if (!g->cv.wait_for(lk, std::chrono::seconds(timeout_s()), [&] { return g->gen != my || g->broken; }) || g->broken) {
        g->broken = true; g->cv.notify_all();
        return false;
    }
    return true;
}

static ncclResult_t get_unique_id(char *id128) {
    memset(id128, 0, 128);
    memcpy(id128, kMagic, 8);
    const unsigned long long n = g_ids.fetch_add(1), pid = (unsigned long long)getpid();
    const unsigned long long t = (unsigned long long)std::chrono::steady_clock::now().time_since_epoch().count();
    memcpy(id128 + 8, &n, 8); memcpy(id128 + 16, &pid, 8); memcpy(id128 + 24, &t, 8);
    return ncclSuccess;
}

static ncclResult_t comm_init(ncclComm_t *out, int world, const char *id128, int rank) {
    if (world < 1 || world > 16 || rank < 0 || rank >= world) return ncclInvalidArgument;
    Group *g;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        const std::string key(id128, 128);
        auto it = g_groups.find(key);
        if (it == g_groups.end()) {
            g = new Group();
            g->id = key; g->world = world;
            g->device.assign(world, -1);
            g->send.assign(world, nullptr); g->ev_ready.assign(world, nullptr); g->ev_done.assign(world, nullptr);
            g->staging.assign(world, nullptr); g->staging_cap.assign(world, 0);
            g->chan.resize((size_t)world * world);
            g_groups[key] = g;
        } else g = it->second;
        if (g->world != world) return ncclInvalidArgument;
        ++g->refs;
    }
    Comm *c = new Comm();
    c->g = g; c->rank = rank; c->rng = 0x9e3779b97f4a7c15ull * (unsigned long long)(rank + 1);
    if (hipEventCreateWithFlags(&g->ev_ready[rank], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&g->ev_done[rank], hipEventDisableTiming) != hipSuccess) return ncclUnhandledCudaError;
    int my_dev = 0;
    if (hipGetDevice(&my_dev) != hipSuccess) return ncclUnhandledCudaError;
    {
        std::unique_lock<std::mutex> lk(g->mu);
        g->device[rank] = my_dev;
        ++g->joined;
        g->cv.notify_all();
        if (!g->cv.wait_for(lk, std::chrono::seconds(timeout_s()), [&] { return g->joined >= g->world; })) return ncclSystemError;
    }
    // slabs on several GPUs of one process: the reduction kernel of a rank reads the staging blocks of the others in place
    for (int r = 0; r < world; ++r)
        if (g->device[r] >= 0 && g->device[r] != my_dev) {
            const hipError_t e = hipDeviceEnablePeerAccess(g->device[r], 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return ncclUnhandledCudaError;
            (void)hipGetLastError();
        }
    { std::lock_guard<std::mutex> lk(g_mu); g_comms.insert(c); }
    *out = (ncclComm_t)c;
    return ncclSuccess;
}

static ncclResult_t comm_destroy(ncclComm_t comm) {
    Comm *c = (Comm *)comm;
    Group *g = c->g;
    // This rank's resources go BEFORE its reference: the rank that drops the last reference deletes the Group, and the ranks of a
    // job close their contexts at the same time from different threads (the first form released the reference first and then
    // touched g->ev_ready: a use-after-free once in a few thousand closes -- tools/fuzz_slabs.py, 1311 cases into a run).
    if (g->ev_ready[c->rank]) hipEventDestroy(g->ev_ready[c->rank]);
    if (g->ev_done[c->rank]) hipEventDestroy(g->ev_done[c->rank]);
    if (g->staging[c->rank]) hipFree(g->staging[c->rank]);
    g->ev_ready[c->rank] = g->ev_done[c->rank] = nullptr; g->staging[c->rank] = nullptr;
    bool last;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        g_comms.erase(c);
        last = --g->refs == 0;
        if (last) g_groups.erase(g->id);
    }
    if (last) {
        for (auto &q : g->chan) for (Msg *m : q) delete m;
        delete g;
    }
    delete c;
    return ncclSuccess;
}

#define LB_HIP(expr) do { if ((expr) != hipSuccess) return ncclUnhandledCudaError; } while (0)

// ---- collectives: every rank of the group executes the same one at the same time ---------------------------------------
static ncclResult_t all_reduce(const Op &o) {
    Comm *c = o.comm; Group *g = c->g; const int W = g->world, me = c->rank;
    const size_t bytes = o.count * dt_size(o.dt);
    const int op = o.op == ncclSum ? 0 : (o.op == ncclMin ? 1 : (o.op == ncclMax ? 2 : -1));
    if (!bytes || op < 0) return ncclInvalidArgument;
    if (g->staging_cap[me] < bytes) {
        // growing: a peer's reduce_kernel of the PREVIOUS reduction may still be reading this block (slabs on several GPUs: the
        // kernel runs on the peer's stream) -- wait for those readers before the block goes (ev_done is recorded by every rank
        // after its reduce kernel; never recorded yet = nothing to wait for)
        if (g->staging[me]) {
            for (int r = 0; r < W; ++r) if (r != me && g->ev_done[r]) (void)hipEventSynchronize(g->ev_done[r]);
            LB_HIP(hipFree(g->staging[me]));
        }
        g->staging[me] = nullptr; g->staging_cap[me] = 0;
        const size_t cap = bytes < 65536 ? 65536 : bytes;
        LB_HIP(hipMalloc(&g->staging[me], cap));
        g->staging_cap[me] = cap;
    }
    jitter(c, o.st);
    LB_HIP(hipMemcpyAsync(g->staging[me], o.src, bytes, hipMemcpyDeviceToDevice, o.st));       // in-place calls: src == dst
    LB_HIP(hipEventRecord(g->ev_ready[me], o.st));
    std::unique_lock<std::mutex> lk(g->mu);
    if (!barrier(g, lk)) return ncclSystemError;
    Ptrs P{};
    for (int r = 0; r < W; ++r) { P.p[r] = g->staging[r]; if (r != me) LB_HIP(hipStreamWaitEvent(o.st, g->ev_ready[r], 0)); }
    const unsigned grid = (unsigned)((o.count + 255) / 256);
    switch (o.dt) {
        case ncclUint32: reduce_kernel<unsigned int><<<grid, 256, 0, o.st>>>(P, W, (unsigned int *)o.dst, o.count, op); break;
        case ncclInt32: reduce_kernel<int><<<grid, 256, 0, o.st>>>(P, W, (int *)o.dst, o.count, op); break;
        case ncclUint64: reduce_kernel<unsigned long long><<<grid, 256, 0, o.st>>>(P, W, (unsigned long long *)o.dst, o.count, op); break;
        case ncclInt64: reduce_kernel<long long><<<grid, 256, 0, o.st>>>(P, W, (long long *)o.dst, o.count, op); break;
        case ncclFloat: reduce_kernel<float><<<grid, 256, 0, o.st>>>(P, W, (float *)o.dst, o.count, op); break;
        default: return ncclInvalidArgument;
    }
    LB_HIP(hipGetLastError());
    LB_HIP(hipEventRecord(g->ev_done[me], o.st));
    if (!barrier(g, lk)) return ncclSystemError;
    for (int r = 0; r < W; ++r) if (r != me) LB_HIP(hipStreamWaitEvent(o.st, g->ev_done[r], 0));     // my staging block is free again
    return ncclSuccess;
}

// all-gather (root < 0): rank r's `count` elements land at dst + r * bytes on every rank; broadcast: root's buffer on every rank
static ncclResult_t gather_or_bcast(const Op &o, int root) {
    Comm *c = o.comm; Group *g = c->g; const int W = g->world, me = c->rank;
    const size_t bytes = o.count * dt_size(o.dt);
    if (!dt_size(o.dt)) return ncclInvalidArgument;
    std::unique_lock<std::mutex> lk(g->mu);
    g->send[me] = o.src;
    LB_HIP(hipEventRecord(g->ev_ready[me], o.st));
    if (!barrier(g, lk)) return ncclSystemError;
    jitter(c, o.st);
    for (int r = 0; r < W; ++r) {
        if (root >= 0 && r != root) continue;
        char *dst = (char *)o.dst + (root < 0 ? (size_t)r * bytes : 0);
        if (r != me) LB_HIP(hipStreamWaitEvent(o.st, g->ev_ready[r], 0));
        if (bytes && (const void *)dst != g->send[r]) LB_HIP(hipMemcpyAsync(dst, g->send[r], bytes, hipMemcpyDeviceToDevice, o.st));
    }
    LB_HIP(hipEventRecord(g->ev_done[me], o.st));
    if (!barrier(g, lk)) return ncclSystemError;
    for (int r = 0; r < W; ++r) if (r != me) LB_HIP(hipStreamWaitEvent(o.st, g->ev_done[r], 0));     // my send buffer has been read
    return ncclSuccess;
}

// ---- a group of operations of one rank: sends are posted first, then everything else in call order, then the sends' streams
// are ordered behind their readers -- no rank blocks in a receive before it has posted what its peers wait for
static ncclResult_t run_ops(std::vector<Op> &ops) {
    for (Op &o : ops) {
        if (o.kind != 0) continue;
        Group *g = o.comm->g;
        if (o.peer < 0 || o.peer >= g->world || o.peer == o.comm->rank) return ncclInvalidArgument;
        Msg *m = new Msg();
        m->src = o.src; m->bytes = o.count * dt_size(o.dt);
        LB_HIP(hipEventCreateWithFlags(&m->ready, hipEventDisableTiming));
        LB_HIP(hipEventCreateWithFlags(&m->done, hipEventDisableTiming));
        LB_HIP(hipEventRecord(m->ready, o.st));
        o.msg = m;
        std::lock_guard<std::mutex> lk(g->mu);
        g->chan[(size_t)o.comm->rank * g->world + o.peer].push_back(m);
        g->cv.notify_all();
    }
    for (Op &o : ops) {
        ncclResult_t r = ncclSuccess;
        if (o.kind == 1) {
            Group *g = o.comm->g;
            if (o.peer < 0 || o.peer >= g->world || o.peer == o.comm->rank) return ncclInvalidArgument;
            Msg *m;
            {
                std::unique_lock<std::mutex> lk(g->mu);
                auto &q = g->chan[(size_t)o.peer * g->world + o.comm->rank];
                if (!g->cv.wait_for(lk, std::chrono::seconds(timeout_s()), [&] { return !q.empty() || g->broken; }) || g->broken) {
                    g->broken = true; g->cv.notify_all();
                    return ncclSystemError;
                }
                m = q.front(); q.pop_front();
            }
            if (m->bytes != o.count * dt_size(o.dt)) r = ncclInvalidArgument;      // sender and receiver disagree on the size
            else {
                LB_HIP(hipStreamWaitEvent(o.st, m->ready, 0));
                jitter(o.comm, o.st);
                if (m->bytes) LB_HIP(hipMemcpyAsync(o.dst, m->src, m->bytes, hipMemcpyDeviceToDevice, o.st));
                LB_HIP(hipEventRecord(m->done, o.st));
            }
            {
                std::lock_guard<std::mutex> lk(g->mu);
                m->consumed = true;
                if (r != ncclSuccess) g->broken = true;
                g->cv.notify_all();
            }
        } else if (o.kind == 2) r = all_reduce(o);
        else if (o.kind == 3) r = gather_or_bcast(o, -1);
        else if (o.kind == 4) r = gather_or_bcast(o, o.peer);
        if (r != ncclSuccess) return r;
    }
    for (Op &o : ops) {
        if (o.kind != 0) continue;
        Group *g = o.comm->g;
        Msg *m = o.msg;
        {
            std::unique_lock<std::mutex> lk(g->mu);
            if (!g->cv.wait_for(lk, std::chrono::seconds(timeout_s()), [&] { return m->consumed || g->broken; }) || g->broken) {
                g->broken = true; g->cv.notify_all();
                return ncclSystemError;
            }
        }
        LB_HIP(hipStreamWaitEvent(o.st, m->done, 0));     // the source planes may be overwritten only after they were read
        hipEventDestroy(m->ready); hipEventDestroy(m->done);
        delete m;
        o.msg = nullptr;
    }
    return ncclSuccess;
}

static ncclResult_t submit(const Op &o) {
    t_ops.push_back(o);
    if (t_depth > 0) return ncclSuccess;
    std::vector<Op> ops;
    ops.swap(t_ops);
    return run_ops(ops);
}
static void group_start() { ++t_depth; }
static ncclResult_t group_end() {
    if (t_depth > 0 && --t_depth > 0) return ncclSuccess;
    if (t_ops.empty()) return ncclSuccess;
    std::vector<Op> ops;
    ops.swap(t_ops);
    return run_ops(ops);
}
#undef LB_HIP
}  // namespace lb
