// pt_group_select.h — what a group of contexts adds to adaptive sampling by threshold (include/pt_amd.h
// pt_group_adaptive_round_threshold), ONE implementation for the kernels (pt_group_select.hip) and for the host function
// (pt_group_partition_host), as pt_adaptive.h is for the selection itself; tests/group_select_ref.py restates the partition in numpy.
//
// A context of a group owns the rows i, i + n, ... of the frame, so neither the 3x3 prefilter of the selection key nor "the cap
// largest keys" can be had from one context's tile.  The frame's selection runs once, on the root device, over what the key reads
// and nothing more: 8 bytes per pixel, {w_p, T_p}.  The frame's list is then cut into one list of tile indices per context.
// Plain C++ apart from PT_HD.
#pragma once
#include <cstddef>
#include <cstdint>

#include "pt_adaptive.h"

namespace ptgs {

constexpr int kMaxParts = 64;  // contexts a list is cut for (pt_amd.h pt_group_partition_host): the kernels keep one counter per part in LDS

// What ptad::key_pixel reads of a pixel, and so what a context sends to the root: plane 0's w and the count plane's T.
struct Packed {
  float w;
  int32_t T;
};
static_assert(sizeof(Packed) == 8, "pt_amd.h documents 8 bytes per pixel on the wire");

template <typename P4>
PT_HD Packed pack_pixel(size_t p, const P4* plane0, const ptad::Cnt* cnt) {
  return Packed{plane0[p].w, cnt[p].T};
}

// The selection key of frame pixel (x, y) from the packed frame: ptad::key_pixel itself, both of its planes being the packed one.
PT_HD uint32_t key_packed(int x, int y, int W, int H, const Packed* frame) { return ptad::key_pixel(x, y, W, H, frame, frame); }

// Frame pixel f of a frame W wide, rows dealt to n contexts in turn: the context that owns it and its index in that context's tile.
PT_HD int owner_of(int32_t f, int W, int n) { return (f / W) % n; }
PT_HD int32_t tile_index(int32_t f, int W, int n) { return ((f / W) / n) * W + f % W; }

// Tile pixel p of a striped tile (runs of `stripe` pixels, `gap` pixels of other tiles between two runs) as an offset from the tile's
// first pixel in the frame: what BatchInfo::list holds (pt_kernels.h), where the merge wants p itself.
PT_HD int32_t stripe_offset(int32_t p, int stripe, int gap) { return p + (p / stripe) * gap; }

// The whole partition on the host: list holds m frame pixels in ascending order; part i receives the tile indices of the pixels
// context i owns, in input order (ascending tile index); the parts lie back to back in `parts`, counts[i] = their lengths.
inline void partition_host(int W, int n, const int32_t* list, int m, int32_t* parts, int32_t* counts) {
  for (int i = 0; i < n; ++i) counts[i] = 0;
  for (int j = 0; j < m; ++j) counts[owner_of(list[j], W, n)] += 1;
  int32_t at[kMaxParts];
  for (int i = 0, sum = 0; i < n; ++i) at[i] = sum, sum += counts[i];
  for (int j = 0; j < m; ++j) parts[at[owner_of(list[j], W, n)]++] = tile_index(list[j], W, n);
}

}  // namespace ptgs
