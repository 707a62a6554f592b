// What the two workspace declarations (infer_workspace.h, train_workspace.h) share: the generators that turn a slot table
// X(slot, pointer member, element type, element count) into the byte layout, the typed pointers and carve(), and the sizes of the
// prepared-weight sub-buffers both workspaces hold.  Host code only.
#pragma once
#include "sir_internal.h"        // sir_align_up

// A table lists its slots in layout order, which is also the order of the published indices: the offset and carve generators walk
// `off` in step with the table.  Every slot starts on a 256-byte boundary; a slot of zero elements takes no bytes.  (The enum
// generator is each header's own: it carries the enum's prefix.)
#define SIR_SLOT_OFFSET(id, member, type, count) *off++ = pos; pos += sir_align_up((size_t)(count) * sizeof(type), 256);
#define SIR_SLOT_MEMBER(id, member, type, count) type* member;
#define SIR_SLOT_CARVE(id, member, type, count) p.member = (type*)(b + *off++);

// ---- sub-buffers of the WS and WCB slots (16-bit elements) and the blocks of the prep jobs that fill them ----
constexpr int prep_blocks(size_t elems, int per_block = 256) { return (int)((elems + per_block - 1) / per_block); }
// WS: f16x2 planes of W_ih, one direction = [2 planes][768][in]; a split2h block covers 2048 weights
constexpr size_t WS_DIR0 = (size_t)2 * 768 * 1024, WS_DIR1 = (size_t)2 * 768 * 512;          // layer 0 / layer 1
constexpr int WS_DIR0_BLOCKS = prep_blocks(768 * 1024, 2048), WS_DIR1_BLOCKS = prep_blocks(768 * 512, 2048);
// WCB: three planes of conv weights per form; one prep thread per weight of a plane
constexpr size_t WCB_W2 = 32 * 16 * 64;        // conv2, 16 Winograd frequencies: the forward's form, and the data gradient's (64 -> 32)
constexpr size_t WCB_W3 = 64 * 16 * 128;       // conv3 likewise (data gradient 128 -> 64)
constexpr size_t WCB_W2_TAPS = 32 * 9 * 64;    // conv2 data gradient with 9 taps (direct fallback; written into the Winograd-sized sub-buffer)
constexpr size_t WCB_W3_TAPS = 64 * 9 * 128;   // conv3 forward with 9 taps (direct fallback)
