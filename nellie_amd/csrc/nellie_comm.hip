// Part of libnellie_hip.so (gfx950): everything that talks to another rank -- the RCCL loader, the loopback transport, the communicator
// pool, the ghost-plane exchange and the collectives of the C-ABI (include/nellie_amd.h), and the small reductions the sampling and
// Filter units put between their kernels (declared in nl_host.h).  Host code, and the one kernel of loopback.inc.
#include "nl_host.h"

// RCCL is loaded on first use (dlopen) instead of being linked: librccl.so is ~570 MB and would be paged in by every
// single-GPU process that merely loads this library.
struct RcclApi {
    void *handle = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclBroadcast) Broadcast = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    bool ok = false;
};
static RcclApi &rccl_real() {
    static RcclApi api;
    if (!api.handle) {
        // The installed ROCm's copy BY PATH first: a bare "librccl.so.1" is answered with whatever object of that SONAME the process
        // already holds -- e.g. the RCCL a PyTorch wheel bundles (built against another HIP runtime: ncclCommInitRank then fails with
        // "unhandled cuda error"; found when a test imported torch into the pytest process, round 5).
        std::string rp;
        if (const char *e = getenv("ROCM_PATH")) rp = std::string(e) + "/lib/librccl.so.1";
        const char *names[] = {rp.c_str(), "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so", "librccl.so.1", "librccl.so"};
        for (const char *n : names) { if (!*n) continue; api.handle = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (api.handle) break; }
        if (api.handle) {
#define NL_SYM(F) api.F = (decltype(api.F))dlsym(api.handle, "nccl" #F)
            NL_SYM(GetUniqueId); NL_SYM(CommInitRank); NL_SYM(CommDestroy); NL_SYM(GetErrorString); NL_SYM(GroupStart);
            NL_SYM(GroupEnd); NL_SYM(Send); NL_SYM(Recv); NL_SYM(AllReduce); NL_SYM(Broadcast); NL_SYM(AllGather);
#undef NL_SYM
            api.ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.GetErrorString && api.GroupStart &&
                     api.GroupEnd && api.Send && api.Recv && api.AllReduce && api.Broadcast && api.AllGather;
        }
    }
    return api;
}

#include "loopback.inc"

// What the entry points call: the same names, dispatched per communicator -- a communicator created from a loopback id
// (nl_comm_loopback_id) lives in loopback.inc, every other one is RCCL's.  librccl.so is only loaded when a real id is asked
// for or used.
static ncclResult_t comm_missing() { return (ncclResult_t)lb::kMissing; }
ncclResult_t CommApi::GetUniqueId(ncclUniqueId *id) { return rccl_real().ok ? rccl_real().GetUniqueId(id) : comm_missing(); }
ncclResult_t CommApi::CommInitRank(ncclComm_t *comm, int world, ncclUniqueId id, int rank) {
    if (lb::is_loopback_id(id.internal)) return lb::comm_init(comm, world, id.internal, rank);
    if (!rccl_real().ok) return comm_missing();
    const ncclResult_t r = rccl_real().CommInitRank(comm, world, id, rank);
    if (r == ncclSuccess) ++n_real;
    return r;
}
ncclResult_t CommApi::CommDestroy(ncclComm_t comm) {
    if (lb::is_ours(comm)) return lb::comm_destroy(comm);
    if (!rccl_real().ok) return comm_missing();
    --n_real;
    return rccl_real().CommDestroy(comm);
}
const char *CommApi::GetErrorString(ncclResult_t r) {
    if ((int)r == lb::kMissing) return "librccl.so could not be loaded";
    if (rccl_real().handle && rccl_real().ok) return rccl_real().GetErrorString(r);
    switch (r) {
        case ncclInvalidArgument: return "invalid argument (loopback transport)";
        case ncclSystemError: return "rendezvous timed out or a peer failed (loopback transport)";
        case ncclUnhandledCudaError: return "HIP error (loopback transport)";
        default: return "error (loopback transport)";
    }
}
ncclResult_t CommApi::GroupStart() {
    lb::group_start();
    return n_real.load() > 0 ? rccl_real().GroupStart() : ncclSuccess;
}
ncclResult_t CommApi::GroupEnd() {
    const ncclResult_t r = lb::group_end();
    const ncclResult_t q = n_real.load() > 0 ? rccl_real().GroupEnd() : ncclSuccess;
    return r != ncclSuccess ? r : q;
}
ncclResult_t CommApi::Send(const void *buf, size_t count, ncclDataType_t dt, int peer, ncclComm_t comm, hipStream_t st) {
    if (lb::is_ours(comm)) return lb::submit(lb::Op{0, buf, nullptr, count, dt, ncclSum, peer, (lb::Comm *)comm, st});
    return rccl_real().Send(buf, count, dt, peer, comm, st);
}
ncclResult_t CommApi::Recv(void *buf, size_t count, ncclDataType_t dt, int peer, ncclComm_t comm, hipStream_t st) {
    if (lb::is_ours(comm)) return lb::submit(lb::Op{1, nullptr, buf, count, dt, ncclSum, peer, (lb::Comm *)comm, st});
    return rccl_real().Recv(buf, count, dt, peer, comm, st);
}
ncclResult_t CommApi::AllReduce(const void *src, void *dst, size_t count, ncclDataType_t dt, ncclRedOp_t op, ncclComm_t comm, hipStream_t st) {
    if (lb::is_ours(comm)) return lb::submit(lb::Op{2, src, dst, count, dt, op, -1, (lb::Comm *)comm, st});
    return rccl_real().AllReduce(src, dst, count, dt, op, comm, st);
}
ncclResult_t CommApi::AllGather(const void *src, void *dst, size_t count, ncclDataType_t dt, ncclComm_t comm, hipStream_t st) {
    if (lb::is_ours(comm)) return lb::submit(lb::Op{3, src, dst, count, dt, ncclSum, -1, (lb::Comm *)comm, st});
    return rccl_real().AllGather(src, dst, count, dt, comm, st);
}
ncclResult_t CommApi::Broadcast(const void *src, void *dst, size_t count, ncclDataType_t dt, int root, ncclComm_t comm, hipStream_t st) {
    if (lb::is_ours(comm)) return lb::submit(lb::Op{4, src, dst, count, dt, ncclSum, root, (lb::Comm *)comm, st});
    return rccl_real().Broadcast(src, dst, count, dt, root, comm, st);
}
CommApi &rccl() { static CommApi api; return api; }

// ---- small reductions on the context stream (nl_comm_fuse), see nl_host.h ------------------------------------------------------
int reduce_range(nl_ctx *c, unsigned int *res, unsigned int *res_b, char *err, size_t errlen) {
    NL_NCCL(rccl().GroupStart());
    for (unsigned int *r : {res, res_b}) {
        if (!r) continue;
        NL_NCCL(rccl().AllReduce(r, r, 1, ncclUint32, ncclMin, (ncclComm_t)c->comm, c->stream));
        NL_NCCL(rccl().AllReduce(r + 1, r + 1, 1, ncclUint32, ncclMax, (ncclComm_t)c->comm, c->stream));
        NL_NCCL(rccl().AllReduce(r + 2, r + 2, 1, ncclUint64, ncclSum, (ncclComm_t)c->comm, c->stream));
    }
    NL_NCCL(rccl().GroupEnd());
    return NL_OK;
}
static int reduce(nl_ctx *c, void *v, size_t n, ncclDataType_t dt, ncclRedOp_t op, char *err, size_t errlen) {
    NL_NCCL(rccl().AllReduce(v, v, n, dt, op, (ncclComm_t)c->comm, c->stream));
    return NL_OK;
}
int reduce_u64_sum(nl_ctx *c, unsigned long long *v, size_t n, char *err, size_t errlen, unsigned long long *v_b) {
    if (!v_b) return reduce(c, v, n, ncclUint64, ncclSum, err, errlen);
    NL_NCCL(rccl().GroupStart());
    for (unsigned long long *p : {v, v_b}) { int rc = reduce(c, p, n, ncclUint64, ncclSum, err, errlen); if (rc) return rc; }
    NL_NCCL(rccl().GroupEnd());
    return NL_OK;
}
int reduce_u32_sum(nl_ctx *c, unsigned int *v, size_t n, char *err, size_t errlen) { return reduce(c, v, n, ncclUint32, ncclSum, err, errlen); }
int reduce_u32_max(nl_ctx *c, unsigned int *v, size_t n, char *err, size_t errlen) { return reduce(c, v, n, ncclUint32, ncclMax, err, errlen); }

extern "C" int nl_comm_unique_id(char *id128, char *err, size_t errlen) {
    if (!id128) return nl_fail(err, errlen, NL_EINVAL, "id buffer is NULL");
    ncclUniqueId id;
    {
        (void)hipGetLastError();        // (see comm_acquire)
        ncclResult_t r_ = rccl().GetUniqueId(&id);
        if (r_ != ncclSuccess) return nl_fail(err, errlen, NL_ECOMM, "ncclGetUniqueId: %s", rccl().GetErrorString(r_));
    }
    static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
    memcpy(id128, &id, 128);
    return NL_OK;
}

// An id of the loopback transport (loopback.inc): `world` contexts of THIS process, one host thread per rank, exchange
// through device-to-device copies on the very streams, with the very offsets and counts RCCL would be given.
extern "C" int nl_comm_loopback_id(char *id128, char *err, size_t errlen) {
    if (!id128) return nl_fail(err, errlen, NL_EINVAL, "id buffer is NULL");
    lb::get_unique_id(id128);
    return NL_OK;
}

// RCCL communicators outlive their context: a context that closes hands its communicators to a per-process pool, and the next
// context of the same (device, world, rank, role) takes them from there instead of creating new ones (every rank does the
// same, so the pool's state is the same everywhere; the id the caller brings is then not used -- the CONSTRAINT: the ranks of a
// job open and close their contexts in the same order, which the SPMD stage classes do; a rank that restarts alone, or a context
// that failed in a collective (its communicators are destroyed instead, `comm_poisoned`), needs fresh ids on every rank).  Why: a process in which an RCCL
// communicator has been destroyed -- or created beside an older one -- runs every later slab step 9-18 % slower (measured at
// world 1 on a 128 x 2048 x 2048 slab: 29.9 -> 32.7 ms synchronous, 30.1 -> 35.3 ms with the device chain; with the earlier
// communicators neither destroyed nor replaced: 30.1), and the stages of a run (Filter, then Label) each open a context.
// Loopback communicators are plain host objects and are destroyed with their context.
struct PooledComm { int device, world, rank, role; ncclComm_t comm; };
static std::mutex g_comm_pool_mu;
static std::vector<PooledComm> g_comm_pool;
static ncclComm_t comm_pool_take(int device, int world, int rank, int role) {
    std::lock_guard<std::mutex> lk(g_comm_pool_mu);
    for (size_t i = 0; i < g_comm_pool.size(); ++i) {
        const PooledComm &p = g_comm_pool[i];
        if (p.device == device && p.world == world && p.rank == rank && p.role == role) {
            ncclComm_t c = p.comm;
            g_comm_pool.erase(g_comm_pool.begin() + (long)i);
            return c;
        }
    }
    return nullptr;
}
void comm_release(nl_ctx *c, void *comm, int role) {
    if (!comm) return;
    // a communicator whose context saw a collective fail may be out of step with its peers: never hand it to a later context
    if (lb::is_ours(comm) || c->comm_poisoned || getenv("NELLIE_DESTROY_COMMS")) { rccl().CommDestroy((ncclComm_t)comm); return; }
    std::lock_guard<std::mutex> lk(g_comm_pool_mu);
    g_comm_pool.push_back(PooledComm{c->device, c->world, c->rank, role, (ncclComm_t)comm});
}
static int comm_acquire(nl_ctx *c, int world, int rank, const char *id128, int role, ncclComm_t *out, char *err, size_t errlen) {
    ncclUniqueId id;
    memcpy(&id, id128, 128);
    if (!lb::is_loopback_id(id128)) {
        ncclComm_t pooled = comm_pool_take(c->device, world, rank, role);
        if (pooled) { *out = pooled; return NL_OK; }
    }
    (void)hipGetLastError();        // RCCL checks the thread's last HIP error during init: it must not inherit one that was handled long ago
    NL_NCCL(rccl().CommInitRank(out, world, id, rank));
    return NL_OK;
}

extern "C" int nl_comm_init(nl_ctx *c, int world, int rank, const char *id128, char *err, size_t errlen) {
    NL_ENTER(c);
    if (!id128 || world < 1 || rank < 0 || rank >= world) return nl_fail(err, errlen, NL_EINVAL, "bad communicator arguments");
    if (c->comm) return nl_fail(err, errlen, NL_ESTATE, "the context already has a communicator");
    ncclComm_t comm;
    int rc = comm_acquire(c, world, rank, id128, 1, &comm, err, errlen);
    if (rc) return rc;
    c->comm = comm; c->world = world; c->rank = rank;
    return NL_OK;
}

// Ghost-plane exchange with the Z neighbours over RCCL (xGMI).  The `depth` owned planes that start `offset` planes inside
// this rank's boundary go to the neighbour's ghost planes at the same distance from the interface, and the neighbours'
// come into ours: low side  send [own_lo + offset, +depth)  recv [own_lo - offset - depth, own_lo - offset),
//                 high side send [own_hi - offset - depth, own_hi - offset)  recv [own_hi + offset, +depth).
// offset 0 = the classic halo.  Asynchronous on the context stream; with `async` != 0 (and a second communicator,
// nl_comm_init2) it runs on a stream and a communicator of its own, ordered after everything submitted so far, and the next
// nl_gauss_step waits for it: the exchange for cascade step s+1 then travels while scale s is being evaluated.
static int halo_exchange_impl(nl_ctx *c, int field, int64_t offset, int64_t depth, int async, char *err, size_t errlen) {
    if (!c->comm) return nl_fail(err, errlen, NL_ESTATE, "nl_halo_exchange before nl_comm_init");
    c->fsq_cache_valid = 0;
    float *p = field_ptr(c, field);
    if (!p) return nl_fail(err, errlen, NL_EINVAL, "nl_halo_exchange: field %d has no volume", field);
    const i64 plane = c->ny * c->nx;
    const bool has_lo = c->rank > 0, has_hi = c->rank + 1 < c->world;
    if (depth < 1 || offset < 0 || offset + depth > c->own_hi - c->own_lo || (has_lo && offset + depth > c->own_lo) ||
        (has_hi && offset + depth > c->nzl - c->own_hi))
        return nl_fail(err, errlen, NL_EINVAL, "halo planes [%lld, %lld) from the interface do not fit the slab (own %lld, ghosts %lld/%lld)", (i64)offset,
                       (i64)(offset + depth), (i64)(c->own_hi - c->own_lo), (i64)c->own_lo, (i64)(c->nzl - c->own_hi));
    const bool side = async && c->comm2;
    ncclComm_t comm = (ncclComm_t)(side ? c->comm2 : c->comm);
    hipStream_t st = c->stream;
    if (side) {
        if (!c->xstream) {
            NL_HIP(hipStreamCreateWithFlags(&c->xstream, hipStreamNonBlocking));
            NL_HIP(hipEventCreateWithFlags(&c->ev_x_main, hipEventDisableTiming));
            NL_HIP(hipEventCreateWithFlags(&c->ev_x_done, hipEventDisableTiming));
        }
        if (c->halo_pending) NL_HIP(hipStreamWaitEvent(c->stream, c->ev_x_done, 0));      // one exchange in flight at a time
        NL_HIP(hipEventRecord(c->ev_x_main, c->stream));
        NL_HIP(hipStreamWaitEvent(c->xstream, c->ev_x_main, 0));
        st = c->xstream;
    }
    ProfScope ps(c, "halo", st);
    NL_NCCL(rccl().GroupStart());
    if (has_lo) {
        NL_NCCL(rccl().Send(p + (c->own_lo + offset) * plane, (size_t)(depth * plane), ncclFloat, c->rank - 1, comm, st));
        NL_NCCL(rccl().Recv(p + (c->own_lo - offset - depth) * plane, (size_t)(depth * plane), ncclFloat, c->rank - 1, comm, st));
    }
    if (has_hi) {
        NL_NCCL(rccl().Send(p + (c->own_hi - offset - depth) * plane, (size_t)(depth * plane), ncclFloat, c->rank + 1, comm, st));
        NL_NCCL(rccl().Recv(p + (c->own_hi + offset) * plane, (size_t)(depth * plane), ncclFloat, c->rank + 1, comm, st));
    }
    NL_NCCL(rccl().GroupEnd());
    if (side) {
        NL_HIP(hipEventRecord(c->ev_x_done, c->xstream));
        c->halo_pending = 1;
    }
    return NL_OK;
}
extern "C" int nl_halo_exchange(nl_ctx *c, int field, int64_t depth, char *err, size_t errlen) {
    NL_ENTER(c);
    return halo_exchange_impl(c, field, 0, depth, 0, err, errlen);
}
extern "C" int nl_halo_exchange_at(nl_ctx *c, int field, int64_t offset, int64_t depth, int async, char *err, size_t errlen) {
    NL_ENTER(c);
    return halo_exchange_impl(c, field, offset, depth, async, err, errlen);
}
// second communicator (its own unique id): carries the asynchronous ghost-plane exchanges, so that they do not serialise
// with the reductions of the first one
extern "C" int nl_comm_init2(nl_ctx *c, int world, int rank, const char *id128, char *err, size_t errlen) {
    NL_ENTER(c);
    if (!id128 || world != c->world || rank != c->rank || !c->comm) return nl_fail(err, errlen, NL_EINVAL, "nl_comm_init2 needs the world / rank of nl_comm_init");
    if (c->comm2) return nl_fail(err, errlen, NL_ESTATE, "the context already has a second communicator");
    ncclComm_t comm;
    int rc = comm_acquire(c, world, rank, id128, 2, &comm, err, errlen);
    if (rc) return rc;
    c->comm2 = comm;
    return NL_OK;
}

// Small all-reduce of host values through RCCL: dtype 0 = int64, 1 = float32; op 0 = sum, 1 = min, 2 = max.
extern "C" int nl_allreduce(nl_ctx *c, void *host_inout, int64_t count, int dtype, int op, char *err, size_t errlen) {
    NL_ENTER(c);
    NL_KEEP_SUPPORT(c);
    if (!c->comm) return nl_fail(err, errlen, NL_ESTATE, "nl_allreduce before nl_comm_init");
    const size_t es = dtype == 0 ? 8 : 4;
    if (!host_inout || count < 1 || (size_t)count * es > (1 << 15) || dtype < 0 || dtype > 1 || op < 0 || op > 2)
        return nl_fail(err, errlen, NL_EINVAL, "bad all-reduce arguments");
    memcpy(c->h_small, host_inout, (size_t)count * es);
    NL_HIP(hipMemcpyAsync(c->d_small, c->h_small, (size_t)count * es, hipMemcpyHostToDevice, c->stream));
    const ncclRedOp_t ops[3] = {ncclSum, ncclMin, ncclMax};
    NL_NCCL(rccl().AllReduce(c->d_small, c->d_small, (size_t)count, dtype == 0 ? ncclInt64 : ncclFloat, ops[op], (ncclComm_t)c->comm, c->stream));
    NL_HIP(hipMemcpyAsync(c->h_small, c->d_small, (size_t)count * es, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    memcpy(host_inout, c->h_small, (size_t)count * es);
    return NL_OK;
}

extern "C" int nl_comm_fuse(nl_ctx *c, int on, char *err, size_t errlen) {
    NL_ENTER(c);
    if (on && !c->comm) return nl_fail(err, errlen, NL_ESTATE, "nl_comm_fuse before nl_comm_init");
    c->fuse_reduce = on ? 1 : 0;
    return NL_OK;
}

// ---- all-gathers of host data ---------------------------------------------------------------------------------------------------
// One growth rule for the staging buffers: half as much again as asked for (the tables of the next phase / frame differ a little).
int ag_reserve(nl_ctx *c, size_t device_bytes, size_t host_bytes, char *err, size_t errlen) {
    if (device_bytes > c->ag_cap) {
        if (c->d_ag) hipFree(c->d_ag);
        c->d_ag = nullptr; c->ag_cap = 0;
        NL_HIP(hipMalloc(&c->d_ag, device_bytes + device_bytes / 2));
        c->ag_cap = device_bytes + device_bytes / 2;
    }
    if (host_bytes > c->h_ag_cap) {
        if (c->h_ag) hipHostFree(c->h_ag);
        c->h_ag = nullptr; c->h_ag_cap = 0;
        NL_HIP(hipHostMalloc(&c->h_ag, host_bytes + host_bytes / 2, hipHostMallocDefault));
        c->h_ag_cap = host_bytes + host_bytes / 2;
    }
    return NL_OK;
}
int allgather_sizes(nl_ctx *c, int64_t nbytes, int64_t *bytes_of, char *err, size_t errlen) {
    long long *hs = (long long *)c->h_small;
    hs[0] = nbytes;
    NL_HIP(hipMemcpyAsync(c->d_small, hs, 8, hipMemcpyHostToDevice, c->stream));
    NL_NCCL(rccl().AllGather(c->d_small, (char *)c->d_small + 64, 1, ncclInt64, (ncclComm_t)c->comm, c->stream));
    NL_HIP(hipMemcpyAsync(hs, (char *)c->d_small + 64, (size_t)c->world * 8, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    for (int r = 0; r < c->world; ++r) bytes_of[r] = hs[r];
    return NL_OK;
}
// the blocks of `block` bytes: this rank's at the start of d_ag, everybody's behind it, downloaded to `recv`; one wait
static int allgather_blocks(nl_ctx *c, const void *send, int64_t nbytes, size_t block, void *recv, char *err, size_t errlen) {
    char *d_send = (char *)c->d_ag, *d_recv = d_send + block;
    if (nbytes) NL_HIP(hipMemcpyAsync(d_send, send, (size_t)nbytes, hipMemcpyHostToDevice, c->stream));
    NL_NCCL(rccl().AllGather(d_send, d_recv, block, ncclChar, (ncclComm_t)c->comm, c->stream));
    NL_HIP(hipMemcpyAsync(recv, d_recv, block * c->world, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    return NL_OK;
}

// Variable-size all-gather of host bytes (see include/nellie_amd.h).  Two collectives: the sizes, then the padded blocks.
extern "C" int nl_allgather_bytes(nl_ctx *c, const void *send, int64_t nbytes, void *recv, int64_t max_bytes, int64_t *bytes_of,
                                  char *err, size_t errlen) {
    NL_ENTER(c);
    NL_KEEP_SUPPORT(c);
    if (!c->comm) return nl_fail(err, errlen, NL_ESTATE, "nl_allgather_bytes before nl_comm_init");
    if (nbytes < 0 || max_bytes < 1 || nbytes > max_bytes || !recv || !bytes_of || (nbytes && !send))
        return nl_fail(err, errlen, NL_EINVAL, "bad all-gather arguments");
    int rc;
    if ((rc = allgather_sizes(c, nbytes, bytes_of, err, errlen))) return rc;
    for (int r = 0; r < c->world; ++r)
        if (bytes_of[r] > max_bytes) return nl_fail(err, errlen, NL_EINVAL, "rank %d sends %lld bytes, more than max_bytes = %lld", r, (long long)bytes_of[r], (long long)max_bytes);
    if ((rc = ag_reserve(c, (size_t)max_bytes * (size_t)(c->world + 1), 0, err, errlen))) return rc;
    return allgather_blocks(c, send, nbytes, (size_t)max_bytes, recv, err, errlen);
}

// The same without a size negotiated by the caller: the block size is the largest of the gathered sizes, and the blocks land
// in a page-locked buffer the context owns (*recv, valid until the next call; rank r's block at r * *stride).
extern "C" int nl_allgather_var(nl_ctx *c, const void *send, int64_t nbytes, void **recv, int64_t *stride, int64_t *bytes_of,
                                char *err, size_t errlen) {
    NL_ENTER(c);
    NL_KEEP_SUPPORT(c);
    if (!c->comm) return nl_fail(err, errlen, NL_ESTATE, "nl_allgather_var before nl_comm_init");
    if (nbytes < 0 || !recv || !stride || !bytes_of || (nbytes && !send)) return nl_fail(err, errlen, NL_EINVAL, "bad all-gather arguments");
    int rc;
    if ((rc = allgather_sizes(c, nbytes, bytes_of, err, errlen))) return rc;
    long long mx = 16;
    for (int r = 0; r < c->world; ++r) if (bytes_of[r] > mx) mx = bytes_of[r];
    mx = (mx + 15) & ~15ll;
    if ((rc = ag_reserve(c, (size_t)mx * (size_t)(c->world + 1), (size_t)mx * c->world, err, errlen))) return rc;
    if ((rc = allgather_blocks(c, send, nbytes, (size_t)mx, c->h_ag, err, errlen))) return rc;
    *recv = c->h_ag; *stride = mx;
    return NL_OK;
}
