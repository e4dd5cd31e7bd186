// comm_rccl.hip -- sfmba_comm_*: RCCL (ncclAllReduce over xGMI) bound at run time: the library has no link-time dependency on librccl
#include "problem.h"

#include <rccl/rccl.h>
#include <dlfcn.h>

using namespace sfmba;

struct sfmba_comm { ncclComm_t comm = nullptr; int rank = 0, world = 1; };
namespace {
struct RcclApi {
    void* handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;
    ncclResult_t (*ReduceScatter)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;
};
RcclApi* rccl() {
    static RcclApi api;
    static bool tried = false;
    if (!tried) {
        tried = true;
        for (const char* name : { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" }) { api.handle = dlopen(name, RTLD_NOW | RTLD_GLOBAL); if (api.handle) break; }
        if (api.handle) {
            api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(dlsym(api.handle, "ncclGetUniqueId"));
            api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(dlsym(api.handle, "ncclCommInitRank"));
            api.AllReduce = reinterpret_cast<decltype(api.AllReduce)>(dlsym(api.handle, "ncclAllReduce"));
            api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(api.handle, "ncclCommDestroy"));
            api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(api.handle, "ncclGetErrorString"));
            api.CommAbort = reinterpret_cast<decltype(api.CommAbort)>(dlsym(api.handle, "ncclCommAbort"));
            api.ReduceScatter = reinterpret_cast<decltype(api.ReduceScatter)>(dlsym(api.handle, "ncclReduceScatter"));
            api.AllGather = reinterpret_cast<decltype(api.AllGather)>(dlsym(api.handle, "ncclAllGather"));
            api.CommCount = reinterpret_cast<decltype(api.CommCount)>(dlsym(api.handle, "ncclCommCount"));
            api.CommUserRank = reinterpret_cast<decltype(api.CommUserRank)>(dlsym(api.handle, "ncclCommUserRank"));
            if (!api.GetUniqueId || !api.CommInitRank || !api.AllReduce || !api.CommDestroy) api.handle = nullptr;
        }
    }
    return api.handle ? &api : nullptr;
}
}  // namespace

extern "C" {
int sfmba_comm_unique_id(unsigned char id[SFMBA_COMM_ID_BYTES]) {
    static_assert(sizeof(ncclUniqueId) == SFMBA_COMM_ID_BYTES, "ncclUniqueId size");
    RcclApi* a = rccl();
    if (!a || !id) return fail(SFMBA_ERR_HIP, "RCCL (librccl.so) is not available");
    ncclUniqueId u;
    const ncclResult_t r = a->GetUniqueId(&u);
    if (r != ncclSuccess) return fail(SFMBA_ERR_HIP, std::string("ncclGetUniqueId: ") + (a->GetErrorString ? a->GetErrorString(r) : "error"));
    std::memcpy(id, &u, sizeof(u));
    return SFMBA_OK;
}

int sfmba_comm_create(const unsigned char id[SFMBA_COMM_ID_BYTES], int rank, int world, int device, sfmba_comm** out) {
    if (!out || !id || world < 1 || rank < 0 || rank >= world) return fail(SFMBA_ERR_INVALID_ARG, "bad argument");
    *out = nullptr;
    RcclApi* a = rccl();
    if (!a) return fail(SFMBA_ERR_HIP, "RCCL (librccl.so) is not available");
    int rc = check_device(device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof(u));
    sfmba_comm* c = new sfmba_comm();
    c->rank = rank; c->world = world;
    const ncclResult_t r = a->CommInitRank(&c->comm, world, u, rank);
    if (r != ncclSuccess) { delete c; return fail(SFMBA_ERR_HIP, std::string("ncclCommInitRank: ") + (a->GetErrorString ? a->GetErrorString(r) : "error")); }
    *out = c;
    return SFMBA_OK;
}

void sfmba_comm_destroy(sfmba_comm* c) {
    if (!c) return;
    RcclApi* a = rccl();
    if (a && c->comm) (void)a->CommDestroy(c->comm);
    delete c;
}

int sfmba_comm_size(const sfmba_comm* c, int* world, int* rank) {
    RcclApi* a = rccl();
    if (!c || !c->comm || !a || !a->CommCount || !a->CommUserRank) return fail(SFMBA_ERR_HIP, "ncclCommCount is not available");
    int n = 0, r = -1;
    ncclResult_t e = a->CommCount(c->comm, &n);
    if (e == ncclSuccess) e = a->CommUserRank(c->comm, &r);
    if (e != ncclSuccess) return fail(SFMBA_ERR_HIP, std::string("ncclCommCount: ") + (a->GetErrorString ? a->GetErrorString(e) : "error"));
    if (world) *world = n;
    if (rank) *rank = r;
    return SFMBA_OK;
}

int sfmba_comm_abort(sfmba_comm* c) {
    RcclApi* a = rccl();
    if (!c || !a || !a->CommAbort) return fail(SFMBA_ERR_HIP, "ncclCommAbort is not available");
    if (c->comm) { (void)a->CommAbort(c->comm); c->comm = nullptr; }
    return SFMBA_OK;
}

int sfmba_comm_allreduce(void* comm, void* device_buf, int64_t n_doubles, void* hip_stream) {
    sfmba_comm* c = static_cast<sfmba_comm*>(comm);
    RcclApi* a = rccl();
    if (!c || !a) return -1;
    const ncclResult_t r = a->AllReduce(device_buf, device_buf, (size_t)n_doubles, ncclDouble, ncclSum, c->comm, static_cast<hipStream_t>(hip_stream));
    return r == ncclSuccess ? 0 : (int)r;
}

int sfmba_comm_allreduce_f32(void* comm, void* device_buf, int64_t n_floats, void* hip_stream) {
    sfmba_comm* c = static_cast<sfmba_comm*>(comm);
    RcclApi* a = rccl();
    if (!c || !a) return -1;
    const ncclResult_t r = a->AllReduce(device_buf, device_buf, (size_t)n_floats, ncclFloat, ncclSum, c->comm, static_cast<hipStream_t>(hip_stream));
    return r == ncclSuccess ? 0 : (int)r;
}

int sfmba_comm_reduce_scatter(void* comm, void* send_buf, void* recv_buf, int64_t n_values, int is_f32, void* hip_stream) {
    sfmba_comm* c = static_cast<sfmba_comm*>(comm);
    RcclApi* a = rccl();
    if (!c || !a || !a->ReduceScatter) return -1;
    const ncclResult_t r = a->ReduceScatter(send_buf, recv_buf, (size_t)n_values, is_f32 ? ncclFloat : ncclDouble, ncclSum, c->comm, static_cast<hipStream_t>(hip_stream));
    return r == ncclSuccess ? 0 : (int)r;
}

int sfmba_comm_allgather(void* comm, void* buf, int64_t bytes_per_rank, void* hip_stream) {
    sfmba_comm* c = static_cast<sfmba_comm*>(comm);
    RcclApi* a = rccl();
    if (!c || !a || !a->AllGather) return -1;
    const ncclResult_t r = a->AllGather(static_cast<char*>(buf) + (size_t)c->rank * (size_t)bytes_per_rank, buf, (size_t)bytes_per_rank, ncclChar, c->comm,
                                        static_cast<hipStream_t>(hip_stream));
    return r == ncclSuccess ? 0 : (int)r;
}
}  // extern "C"
