// skml_comm.cpp -- RCCL all-gather of payloads over xGMI (include/skml.h, skml_comm_*).
#include <rccl/rccl.h>

#include <cstring>

#include "skml_host.hpp"

using namespace skml;

extern "C" {

struct skml_comm {
    ncclComm_t comm;
    int nranks, rank;
};

int skml_comm_unique_id(uint8_t id_out[SKML_UNIQUE_ID_BYTES]) {
    static_assert(sizeof(ncclUniqueId) <= SKML_UNIQUE_ID_BYTES, "unique id size");
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return fail(SKML_E_RCCL, "ncclGetUniqueId: %s", ncclGetErrorString(r));
    std::memset(id_out, 0, SKML_UNIQUE_ID_BYTES);
    std::memcpy(id_out, &id, sizeof(id));
    return SKML_OK;
}

int skml_comm_init_rank(skml_ctx* c, const uint8_t id_in[SKML_UNIQUE_ID_BYTES], int32_t nranks,
                        int32_t rank, skml_comm** out) {
    if (!c || !out || nranks < 1 || rank < 0 || rank >= nranks) return fail(SKML_E_ARG, "bad comm args");
    HIP_TRY(hipSetDevice(c->device));
    ncclUniqueId id;
    std::memcpy(&id, id_in, sizeof(id));
    skml_comm* cm = new skml_comm();
    ncclResult_t r = ncclCommInitRank(&cm->comm, nranks, id, rank);
    if (r != ncclSuccess) {
        delete cm;
        return fail(SKML_E_RCCL, "ncclCommInitRank: %s", ncclGetErrorString(r));
    }
    cm->nranks = nranks;
    cm->rank = rank;
    *out = cm;
    return SKML_OK;
}

int skml_comm_destroy(skml_comm* cm) {
    if (!cm) return SKML_OK;
    ncclCommDestroy(cm->comm);
    delete cm;
    return SKML_OK;
}

int skml_allgather(skml_ctx* c, skml_comm* cm, const void* payload, size_t bytes, void* all) {
    if (!c || !cm || !payload || !all) return fail(SKML_E_ARG, "bad allgather arguments");
    HIP_TRY(hipSetDevice(c->device));
    ncclResult_t r = ncclAllGather(payload, all, bytes, ncclUint8, cm->comm, c->stream);
    if (r != ncclSuccess) return fail(SKML_E_RCCL, "ncclAllGather: %s", ncclGetErrorString(r));
    return SKML_OK;
}

}  // extern "C"
