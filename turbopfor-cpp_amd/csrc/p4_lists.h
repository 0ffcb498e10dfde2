// p4_lists.h -- decode and encode of many posting lists laid end to end in one
// call (tpf_p4ndec256v32_lists / tpf_p4nenc256v32_lists, include/turbopfor_gpu.h):
// what the plan pass leaves in the workspace for the kernels after it (internal).
//
// Passes (p4_lists.hip): plan (one thread per list: unit
// counts, structure check) -> run scan of the unit counts (p4_scan.h) -> heads
// (unit bases, one record per unit) -> [delta-1: phase A over every full block
// (k_dsum256v32_lists, p4_dec256v32.hip), its run scan, one prefix per list]
// -> decode (k_lists_dec).  Nothing comes back to the host in between: every
// kernel after the plan reads the header below and does nothing when the list
// structure was refused.  The device helpers the lists kernels share are in
// p4_lists_dev.h (the tails driver among them) and p4_lists_items.h (the item
// drivers), the host ones (grids, the launch helpers) in p4_lists_host.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tpf_ws.h"

namespace tpf
{

// A resident index as the entry points are handed it: the stream and its unit
// offsets, the lists' CSR pointers, the unit directory (tpf_lists_unit_base)
// and, for a delta-1 stream, the lists' starts and the skip table
// (tpf_lists_unit_last; values, never indices).  An entry that does not take a
// member leaves it null; a plain stream has neither start0 nor unit_last.
struct ListsIndex
{
    const uint8_t * in;
    uint64_t in_bytes;
    const uint64_t * off;
    uint64_t nunits;
    const uint64_t * ptr;
    const uint32_t * list_unit;
    uint64_t nlists;
    const uint32_t * start0;
    const uint32_t * unit_last;
};

} // namespace tpf

namespace tpf::dev
{

// Unit record (u32 per unit of the stream): the first unit of list j carries
// j + 1 in the low 31 bits (0: not a head), the p4Enc32 tail of a list carries
// kRecTail.  A tail-only list is both.  A wave finds the list of every unit of
// its run from one search for the run's first unit and a max-scan of the heads.
constexpr uint32_t kRecTail = 0x80000000u;
constexpr uint32_t kRecList = 0x7FFFFFFFu;

// bytes of d_out one wave of the stitch pass moves (p4_lists_stitch.h: the append and the remove)
constexpr uint32_t kListsAppendTile = 16384;

struct ListsHdr
{
    unsigned long long bad;   // first list j with ptr[j+1] < ptr[j] or ptr[j+1] > out_values (~0: none)
    unsigned long long total; // sum of the lists' unit counts
};

// go / no-go: the structure is sound and the unit counts add up to nunits
__device__ __forceinline__ bool lists_go(const ListsHdr * h, uint64_t nunits)
{
    return h->bad == ~0ull && h->total == nunits;
}

// Header of a decode over a SELECTION of a resident index's lists or unit
// ranges (p4_lists_select.hip, p4_lists_units.hip).
struct SelHdr
{
    unsigned long long bad;    // first refused selection k (~0: none)
    unsigned long long vtotal; // virtual units: the sum of the selections' unit counts
    unsigned long long ototal; // selected values: d_out_ptr[nsel]
};

// go / no-go: every selection is sound and the selected values fit the output
// (then vtotal <= vcap follows, n values holding at most n/256 + 1 units; it
// is checked all the same: vcap sizes the records and the sums)
__device__ __forceinline__ bool sel_go(const SelHdr * h, uint64_t out_values, uint64_t vcap)
{
    return h->bad == ~0ull && h->ototal <= out_values && h->vtotal <= vcap;
}

// Header of a request served item by item (p4_lists_items.hip: the
// intersection and the gather).  An ITEM is a run of consecutive request
// indices that name one list and one source unit.
struct ItemHdr
{
    unsigned long long bad; // first refused query k, or a code past nq of the entry's own (~0: none)
    uint32_t nitems;
    uint32_t spare;         // the intersection: nhits = d_out_ptr[nq]; the union and the difference: their misses
};

// go / no-go of everything after the plan: nothing was refused
__device__ __forceinline__ bool items_go(const ItemHdr * h) { return h->bad == ~0ull; }

constexpr uint32_t kItemNone = 0xFFFFFFFFu; // unit word / list word: the request index names nothing

// What the lookup kernels of the intersection read and leave (k_ix_dec /
// k_ix_tails, p4_lists_intersect.hip; the union runs them too).  Result word
// of the intersection's lookup: p inside the unit for a member, else kItemNone.
// Of the union's (EVERY): for every probe value that has a unit, the lower
// bound q of the value over the unit (0 .. 256) in bits 0-8 and kIxFound for a
// member; kItemNone stays where no unit holds the value.
constexpr uint32_t kIxQ = 0x1FFu;
constexpr uint32_t kIxFound = 0x200u;

// What the item drivers read (p4_lists_items.h): the index, the request's plan
// and the items.  IxArgs and GaArgs embed it.
struct ItemArgs
{
    ListsIndex ix;
    const ItemHdr * hdr;
    const uint32_t * pu;    // per request index: source unit | kRecTail, or kItemNone
    const uint32_t * pl;    // per request index: target list, or kItemNone
    const uint32_t * ihead; // per item: its first request index ...
    const uint32_t * iend;  // ... and one past its last
    unsigned long long * err;
};

struct IxArgs
{
    ItemArgs it;            // hdr->spare: the entry's own total
    const uint32_t * probe;
    uint64_t pv;            // probe_values
    uint32_t * res;         // per probe value: the result word (above)
};

} // namespace tpf::dev

namespace tpf
{

size_t lists_workspace(uint64_t nunits, uint64_t nlists);
// The passes the decode and the encode (p4_lists_enc.hip) share: header reset,
// plan, run scan of the lists' unit counts, heads.  `values`: the length of
// the value array the pointers index (out_values / in_values).  `scan` covers
// nlists entries, ubase nlists + 1, rec nunits.  A refused structure is
// reported through `err`.
hipError_t launch_lists_structure(const uint64_t * ptr, uint64_t nlists, uint64_t values, uint64_t nunits, dev::ListsHdr * hdr,
                                  const RunScanWs<uint64_t> & scan, uint32_t * ubase, uint32_t * rec, unsigned long long * err,
                                  hipStream_t s);
// the many-lists encode (p4_lists_enc.hip)
size_t lists_enc_workspace(uint64_t nunits, uint64_t nlists);
hipError_t launch_lists_enc(const uint32_t * in, uint64_t in_values, const uint64_t * ptr, uint64_t nlists, bool d1,
                            const uint32_t * start0, uint8_t * out, uint64_t out_cap, uint64_t * off, uint64_t nunits, void * ws,
                            unsigned long long * err, hipStream_t s);
// the same passes over lists planned on the device (p4_lists_enc.hip): the
// caller fills the view -- header, ubase (nlists + 1), unit records -- and
// units_cap bounds the unit count, which the header holds
struct ListsEncPlanView
{
    dev::ListsHdr * hdr;
    uint32_t * ubase;
    uint32_t * rec;
};
ListsEncPlanView lists_enc_plan_view(void * ws, uint64_t units_cap, uint64_t nlists);
hipError_t launch_lists_enc_planned(const uint32_t * in, const uint64_t * ptr, uint64_t nlists, bool d1, const uint32_t * start0,
                                    uint8_t * out, uint64_t out_cap, uint64_t * off, uint64_t units_cap, void * ws, hipStream_t s);
hipError_t launch_lists_dec(const ListsIndex & X, bool d1, uint32_t * out, uint64_t out_values, void * ws, unsigned long long * err,
                            hipStream_t s);
// the read side of a resident index (p4_lists_select.hip): the
// unit directory of a stream, and the decode of a selection of its lists.
// Passes of the selective decode: plan over the SELECTION -> two run scans
// (virtual unit bases, d_out_ptr) -> heads (records of the virtual units) ->
// [delta-1: block sums of the virtual units, their run scan, one prefix per
// selection] -> full blocks -> tails.  vcap = lists_select_unit_cap: the most
// units a selection that fits out_values can hold; it sizes grids and workspace.
size_t lists_unit_base_workspace(uint64_t nlists);
hipError_t launch_lists_unit_base(const uint64_t * ptr, uint64_t nlists, uint32_t * list_unit, void * ws, unsigned long long * err,
                                  hipStream_t s);
uint64_t lists_select_unit_cap(uint64_t nsel, uint64_t out_values);
size_t lists_select_workspace(uint64_t nsel, uint64_t out_values);
hipError_t launch_lists_select(const ListsIndex & X, bool d1, const uint32_t * sel, uint64_t nsel, uint32_t * out, uint64_t out_values,
                               uint64_t * out_ptr, void * ws, unsigned long long * err, hipStream_t s);
// block-range reads of a resident index (p4_lists_units.hip):
// the skip table of a delta-1 stream (the last value of every unit), the
// search from doc-id ranges to unit ranges, and the decode of unit ranges of
// selected lists.  Passes of the build: structure -> phase A and its run scan
// -> one prefix per list -> the tails' sums -> the write pass.  Passes of the
// decode: plan over the SELECTION -> two run scans -> heads -> full blocks ->
// tails, the same for delta-1 (a unit starts from the table) and plain.
size_t lists_unit_last_workspace(uint64_t nunits, uint64_t nlists);
hipError_t launch_lists_unit_last(const ListsIndex & X, uint32_t * unit_last, void * ws, unsigned long long * err, hipStream_t s);
// the passes the selective decode and the units decode share after their plan
// kernels (p4_lists_select.hip): the two run scans (hdr->vtotal, hdr->ototal)
// and the heads (the verdict, d_out_ptr, vbase, the virtual units' records)
hipError_t launch_sel_heads(uint64_t nsel, uint64_t nunits, uint64_t out_values, uint64_t vcap, dev::SelHdr * hdr,
                            const RunScanWs<uint64_t> & scanu, const uint64_t * totv, uint64_t * prev, uint64_t * tilev, uint32_t * vbase,
                            uint32_t * rec, uint64_t * out_ptr, unsigned long long * err, hipStream_t s);
hipError_t launch_lists_range_units(const uint32_t * list_unit, const uint32_t * unit_last, uint64_t nlists, uint64_t nunits,
                                    const uint32_t * qlist, const uint32_t * qlo, const uint32_t * qhi, uint64_t nq, uint32_t * ufirst,
                                    uint32_t * ucount, unsigned long long * err, hipStream_t s);
size_t lists_units_workspace(uint64_t nsel, uint64_t out_values);
hipError_t launch_lists_units(const ListsIndex & X, bool d1, const uint32_t * sel, const uint32_t * ufirst, const uint32_t * ucount,
                              uint64_t nsel, uint32_t * out, uint64_t out_values, uint64_t * out_ptr, void * ws, unsigned long long * err,
                              hipStream_t s);
// membership of probe values in resident lists (p4_lists_intersect.hip;
// DESIGN.md 4.11).  Passes: plan (one thread per query: the checks; one per
// probe value: its query, then its unit by a search over the skip table) ->
// item heads and their run scan -> items (runs of probe values with one list
// and one unit) -> full blocks -> tails (each item's unit decoded into LDS and
// searched, never stored) -> hit flags and their run scan -> compaction
// (d_out_ptr, the verdict, the scatter).  Sized by nq and probe_values alone.
size_t lists_intersect_workspace(uint64_t nq, uint64_t probe_values);
hipError_t launch_lists_intersect(const ListsIndex & X, const uint32_t * probe, uint64_t probe_values, const uint64_t * probe_ptr,
                                  const uint32_t * qlist, uint64_t nq, uint32_t * out, uint64_t out_values, uint64_t * out_ptr,
                                  uint32_t * out_pidx, uint32_t * out_tpos, void * ws, unsigned long long * err, hipStream_t s);
// the intersection's plan and its lookup (full blocks, tails) for other entries: `every` runs the EVERY
// form of the lookup (dev::kIxFound above); pu / pl / ihead / iend / res as the item layer below leaves them
hipError_t launch_ix_plan(const ListsIndex & X, const uint32_t * probe, uint64_t pv, const uint64_t * probe_ptr, const uint32_t * qlist,
                          uint64_t nq, dev::ItemHdr * hdr, uint32_t * pu, uint32_t * pl, hipStream_t s);
hipError_t launch_ix_lookup(const dev::IxArgs & A, bool every, hipStream_t s);
// the item layer the intersection and the gather share (p4_lists_items.hip).  pu / pl: per request index
// its source unit | kRecTail and its list, or kItemNone (the entry's plan).
// launch_items_reset: d_err and the header's verdict in one launch.
// launch_items: item heads (res != nullptr: every result word starts as
// kItemNone) -> run scan of the 64-index runs (hdr->nitems) -> items (ihead /
// iend: every item's first request index and one past its last).
hipError_t launch_items_reset(unsigned long long * err, dev::ItemHdr * hdr, hipStream_t s);
hipError_t launch_items(uint64_t pv, dev::ItemHdr * hdr, const uint32_t * pu, const uint32_t * pl, const RunScanWs<uint32_t> & scan,
                        uint32_t * ihead, uint32_t * iend, uint32_t * res, hipStream_t s);
// values at given list positions of a resident index (p4_lists_gather.hip;
// DESIGN.md 4.12): the intersection's positional twin, for delta-1 and plain
// streams.  Passes: plan (one thread per query: the checks; one per request
// index: its query, the position against n_j, its unit) -> item heads and their
// run scan -> items -> full blocks -> tails (each item's unit decoded into LDS,
// out[i] = vals[pos[i] % 256]; the tails kernel also writes the verdict of a
// refusal).  Sized by pos_values alone.
size_t lists_gather_workspace(uint64_t nq, uint64_t pos_values);
hipError_t launch_lists_gather(const ListsIndex & X, bool d1, const uint32_t * pos, uint64_t pos_values, const uint64_t * pos_ptr,
                               const uint32_t * qlist, uint64_t nq, uint32_t * out, void * ws, unsigned long long * err, hipStream_t s);
// the sorted union of probe values with resident lists (p4_lists_union.hip;
// DESIGN.md 4.16).  Passes: the intersection's plan, items and lookup (EVERY:
// q and the member flag of every probe value) -> miss flags and their run scan
// -> plan over the QUERIES (n_j + M_k, the units) and two run scans -> heads
// (the verdict, d_out_ptr, the virtual units of the targeted lists) -> misses
// (v to slot L + M, L to the per-query array mlb) -> full blocks -> tails (each
// list value shifted by the misses at or before it) -> the hits' pidx.  Sized
// by nq, probe_values and out_values alone.
size_t lists_union_workspace(uint64_t nq, uint64_t probe_values, uint64_t out_values);
hipError_t launch_lists_union(const ListsIndex & X, const uint32_t * probe, uint64_t probe_values, const uint64_t * probe_ptr,
                              const uint32_t * qlist, uint64_t nq, uint32_t * out, uint64_t out_values, uint64_t * out_ptr,
                              uint32_t * out_pidx, uint32_t * out_tpos, void * ws, unsigned long long * err, hipStream_t s);
// the probe values that are NOT in resident lists (p4_lists_difference.hip;
// DESIGN.md 4.17).  Passes: the intersection's plan, items and lookup (EVERY:
// q and the member flag of every probe value that has a unit) -> miss flags
// (a value without a unit is a miss by the plan's word) and their run scan ->
// compaction (d_out_ptr, the verdict, the scatter of value, probe index and
// L).  Sized by probe_values alone, as the intersection.
size_t lists_difference_workspace(uint64_t nq, uint64_t probe_values);
hipError_t launch_lists_difference(const ListsIndex & X, const uint32_t * probe, uint64_t probe_values, const uint64_t * probe_ptr,
                                   const uint32_t * qlist, uint64_t nq, uint32_t * out, uint64_t out_values, uint64_t * out_ptr,
                                   uint32_t * out_pidx, uint32_t * out_tpos, void * ws, unsigned long long * err, hipStream_t s);
// postings appended to the lists of a resident index (p4_lists_append.hip;
// DESIGN.md 4.13).  Passes: plan (one thread per output list: the checks, what
// of its old tail is staged, its new units) -> four run scans -> heads (the
// verdict, both directories, the staged lists) -> stage (the additions, the old
// tails decoded in front of them) -> the encoder's passes over the staged lists
// -> segs (every list's first output byte, the capacity) -> offsets (d_off_out,
// d_unit_last_out) -> stitch (a wave per kListsAppendTile bytes of d_out).
// Sized by nunits, nlists_out and add_values alone.
size_t lists_append_workspace(uint64_t nunits, uint64_t nlists_out, uint64_t add_values);
hipError_t launch_lists_append(ListsIndex X, bool d1, const uint32_t * add, uint64_t add_values, const uint64_t * aptr, uint64_t nlists_out,
                               uint8_t * out, uint64_t out_cap, uint64_t * off_out, uint64_t units_cap, uint64_t * lptr_out,
                               uint32_t * lunit_out, uint32_t * ulast_out, void * ws, unsigned long long * err, hipStream_t s);
// postings deleted at list positions of a resident index (p4_lists_remove.hip;
// DESIGN.md 4.18).  Passes: plan over the QUERIES (the checks, the unit range
// [u0, end) of every targeted list, its compacted count) and over the positions
// -> plan over the lists (structure, kept units and bytes) -> five run scans ->
// the units decode of the ranges (launch_lists_units) -> heads over the queries
// (the encoder's plan) and over the lists (the verdict, both directories) ->
// compaction -> the encoder's passes -> segs -> offsets -> stitch
// (p4_lists_stitch.h), the last three as the append's.  Workspace, decode and
// encoder are sized by nq and stage_values, the per-list arrays by nlists.
size_t lists_remove_workspace(uint64_t nlists, uint64_t nq, uint64_t stage_values);
hipError_t launch_lists_remove(const ListsIndex & X, bool d1, const uint32_t * pos, uint64_t pos_values, const uint64_t * pos_ptr,
                               const uint32_t * qlist, uint64_t nq, uint64_t stage_values, uint8_t * out, uint64_t out_cap,
                               uint64_t * off_out, uint64_t units_cap, uint64_t * lptr_out, uint32_t * lunit_out, uint32_t * ulast_out,
                               void * ws, unsigned long long * err, hipStream_t s);
// a sub-index of a resident index, moved as bytes (p4_lists_extract.hip;
// DESIGN.md 4.22).  Passes: plan over the SELECTION (the checks, the units,
// values and bytes of every selected unit range) -> three run scans -> heads
// (the verdict, both directories, the delta-1 starts, every selection's first
// output byte, the capacity) -> offsets (d_off_out, d_unit_last_out) -> move
// (stitch_tile, p4_lists_stitch.h, with no new bytes).  The workspace and the
// plan are sized by nsel alone, the offsets by units_cap, the move by out_cap.
size_t lists_extract_workspace(uint64_t nsel);
hipError_t launch_lists_extract(const ListsIndex & X, bool d1, const uint32_t * sel, const uint32_t * ufirst, const uint32_t * ucount,
                                uint64_t nsel, uint8_t * out, uint64_t out_cap, uint64_t * off_out, uint64_t units_cap, uint64_t * lptr_out,
                                uint32_t * lunit_out, uint32_t * start0_out, uint32_t * ulast_out, void * ws, unsigned long long * err,
                                hipStream_t s);
// the unit offsets of a stream that has none, from the lists' byte spans and
// the units' headers (p4_lists_scan.hip).  Passes: plan (one
// thread per list: the checks, its unit count) -> run scan -> short (the
// verdict, the unit directory, the one-unit lists) -> walk (a wave per list of
// two or more units).  The workspace is sized by nlists alone.
size_t lists_unit_offsets_workspace(uint64_t nunits, uint64_t nlists);
hipError_t launch_lists_unit_offsets(const uint8_t * in, uint64_t in_bytes, const uint64_t * ptr, const uint64_t * lbyte, uint64_t nlists,
                                     uint64_t * off, uint64_t nunits, uint32_t * list_unit, void * ws, unsigned long long * err,
                                     hipStream_t s);
// phase A over a lists stream (p4_dec256v32.hip): block sums + run scan into
// `ws` (the chained decode's layout, d1chain_workspace(nunits) bytes), tail
// units skipped; *view = where phase B finds them
struct ChainView
{
    const uint32_t *sums = nullptr, *pre = nullptr, *tile = nullptr;
};
hipError_t launch_lists_sums(const ListsIndex & X, const uint32_t * rec, const dev::ListsHdr * hdr, void * ws, ChainView * view,
                             unsigned long long * err, hipStream_t stream);

} // namespace tpf
