// pt_camera_tables_device.h — the launches of pt_camera_tables.hip, on raw device pointers and a stream; asynchronous, nothing allocated.
// Shared by the translation units of libpt_amd.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "pt_camera_tables.h"
#include "pt_device.h"

// nodes, top and (args.center_half) their centre / half extent copies from the device copy of pt::CameraBase; *rec is zeroed first and
// receives the count of tightened leaves.
int pt_camera_tables_nodes_launch(hipStream_t stream, const ptct::BuildArgs& args, const ptd::Node* base_nodes, const ptd::TopEntry* base_top,
                                  const ptct::DeviceGeom* geoms, ptd::Node* nodes, ptd::Node* nodes_b, ptd::TopEntry* top, ptd::TopEntry* top_b,
                                  ptct::BuildRecord* rec);
// The grid, first half: count (args.ncell words) receives the records per cell, *rec the references and the longest list.  When the
// references exceed ptct::kMaxRefs nothing is counted.
int pt_camera_tables_count_launch(hipStream_t stream, const ptct::BuildArgs& args, const ptd::Node* nodes, uint32_t* count, ptct::BuildRecord* rec);
// The grid, second half, for the `refs` references the first half counted: start (args.ncell + 1 + 2 * args.guard words), items and
// (args.center_half) items_b (refs records each).  sums: pt_camera_tables_scan_blocks(args.ncell) words, scratch: refs words.
size_t pt_camera_tables_scan_blocks(size_t ncell);
int pt_camera_tables_grid_launch(hipStream_t stream, const ptct::BuildArgs& args, const ptd::Node* nodes, const ptct::DeviceGeom* geoms, uint32_t* count,
                                 uint32_t* sums, uint32_t* scratch, uint32_t refs, uint32_t* start, ptd::Node* items, ptd::Node* items_b);
// pt_selfcheck_camera_math on the current device (synchronous; its buffers are scratch)
int pt_camera_math_check(int kind, uint64_t count, uint32_t seed, uint64_t* mismatches);
