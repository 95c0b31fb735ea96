// Internal, not exported: what zkwg_multi_api.hip needs from a handle beyond include/zkwg.h (defined in zkwg_hostpath_api.hip).
// The two batch calls leave every email's result rows {w[1..3]}, 96 bytes, in device memory (`d_rows`, optional) for the gather.
#pragma once
#include "../../include/zkwg.h"
#define ZK_INTERNAL extern "C" __attribute__((visibility("hidden")))
ZK_INTERNAL int zk_calculate_batch_rows(zkwg_circuit_t* c, const uint8_t* packed, uint64_t n, uint8_t* out_wtns, uint64_t out_stride,
                                        int32_t* status, uint64_t max_tile, uint8_t* d_rows);
ZK_INTERNAL int zk_calculate_batch_resident_rows(zkwg_circuit_t* c, const uint8_t* packed, uint64_t n, int32_t* status, uint64_t tile_req,
                                                 uint64_t prep_req, uint8_t* d_rows, zkwg_tile_fn consumer, void* user);
ZK_INTERNAL void* zk_circuit_stream(zkwg_circuit_t* c);      // the handle's own stream
