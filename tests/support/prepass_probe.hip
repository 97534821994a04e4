// prepass_probe.hip -- TEST SUPPORT: the pre-pass kernels (psk_gather.hip, psk_tune.hip, psk_resample.hip, psk_fir.hip), the two
// looks (psk_symrate.hip, psk_acquire.hip: fold and join) and the word search (psk_sync.hip: fold and join) launched by themselves,
// so that tests can hold every byte they write -- each
// row sample, both history slots, every partial and record -- and every byte they must not write to the models, bit for bit
// (tests/prepass_probe.py, tests/test_gpu_prepass_probe.py).
//
// This file holds no kernel.  It is linked with the product's own objects psk_gather.o, psk_tune.o, psk_resample.o, psk_fir.o,
// psk_symrate.o, psk_acquire.o and psk_sync.o as the product's build made them (psk_soft_amd/csrc/Makefile, target ../libpsk_prepass_probe.so): the machine code under test is
// the product's.  Nothing of it is linked into the product library.
//
// One C entry per kernel.  The caller passes one host ARENA -- sources, destination rows, histories, poison everywhere else --
// and descriptors of the product's layout that hold byte offsets into the arena where the product's hold pointers.  An entry
// refuses an offset outside the arena (hipErrorInvalidValue; the extents behind the offsets are the caller's to check),
// allocates a device arena, uploads the host's, turns the offsets into pointers, uploads the descriptors, launches once through
// the product's launch function on a stream of its own, synchronises, downloads the WHOLE arena into the host's and returns the
// HIP status.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "psk_acquire.h"
#include "psk_fir.h"
#include "psk_gather.h"
#include "psk_resample.h"
#include "psk_symrate.h"
#include "psk_sync.h"
#include "psk_tune.h"

using namespace psk;

namespace {

struct Run {
    char *d_arena = nullptr;
    void *d_desc[2] = {nullptr, nullptr};
    float *d_tab = nullptr;
    hipStream_t stream = nullptr;
    hipError_t err = hipSuccess;

    bool ok(hipError_t e)
    {
        if (err == hipSuccess && e != hipSuccess)
            err = e;
        return err == hipSuccess;
    }
    bool begin(const void *arena, uint64_t bytes)
    {
        return ok(hipStreamCreate(&stream)) && ok(hipMalloc((void **)&d_arena, bytes)) &&
               ok(hipMemcpy(d_arena, arena, bytes, hipMemcpyHostToDevice));
    }
    bool descriptors(int k, const void *host, size_t bytes)
    {
        return ok(hipMalloc(&d_desc[k], bytes ? bytes : 16)) && (!bytes || ok(hipMemcpy(d_desc[k], host, bytes, hipMemcpyHostToDevice)));
    }
    bool tables()
    {
        return ok(hipMalloc((void **)&d_tab, sizeof(float) * kTuneTableFloats)) &&
               ok(hipMemcpy(d_tab, tune_tables(), sizeof(float) * kTuneTableFloats, hipMemcpyHostToDevice));
    }
    // behind the launch: wait, bring the arena (and the device's copy of the tables) back, release everything
    int end(hipError_t launched, void *arena, uint64_t bytes, float *tables_out)
    {
        if (ok(launched) && ok(hipStreamSynchronize(stream)) && ok(hipMemcpy(arena, d_arena, bytes, hipMemcpyDeviceToHost)) && tables_out && d_tab)
            ok(hipMemcpy(tables_out, d_tab, sizeof(float) * kTuneTableFloats, hipMemcpyDeviceToHost));
        if (d_tab) (void)hipFree(d_tab);
        for (void *p : d_desc)
            if (p) (void)hipFree(p);
        if (d_arena) (void)hipFree(d_arena);
        if (stream) (void)hipStreamDestroy(stream);
        return (int)err;
    }
};

// an offset of a descriptor as the pointer it stands for; false outside the arena
template <class P>
bool point(P &field, const char *d_arena, uint64_t bytes)
{
    const uint64_t off = (uint64_t)(uintptr_t)field;
    if (off >= bytes)
        return false;
    field = (P)(d_arena + off);
    return true;
}

}  // namespace

extern "C" {

// 0 GatherGroup, 1 GatherChan, 2 GatherSingle, 3 TuneDesc, 4 ResampleDesc, 5 FirDesc, 6 SymrateDesc, 7 SymratePartial, 8 AcquireDesc,
// 9 AcquirePartial, 10 psk_soft_symrate_t, 11 psk_soft_acquire_t, 12 SyncDesc, 13 SyncPartial, 14 psk_soft_sync_t
int psk_prepass_probe_sizeof(int which)
{
    switch (which) {
    case 0: return (int)sizeof(GatherGroup);
    case 1: return (int)sizeof(GatherChan);
    case 2: return (int)sizeof(GatherSingle);
    case 3: return (int)sizeof(TuneDesc);
    case 4: return (int)sizeof(ResampleDesc);
    case 5: return (int)sizeof(FirDesc);
    case 6: return (int)sizeof(SymrateDesc);
    case 7: return (int)sizeof(SymratePartial);
    case 8: return (int)sizeof(AcquireDesc);
    case 9: return (int)sizeof(AcquirePartial);
    case 10: return (int)sizeof(psk_soft_symrate_t);
    case 11: return (int)sizeof(psk_soft_acquire_t);
    case 12: return (int)sizeof(SyncDesc);
    case 13: return (int)sizeof(SyncPartial);
    case 14: return (int)sizeof(psk_soft_sync_t);
    default: return -1;
    }
}

// 0 kResamplePiece, 1 kResampleInputs, 2 kGatherTile, 3 kGatherMinGroup, 4 kTuneTableFloats, 5 kFirWindow, 6 kFirMaxTaps,
// 7 kFirHistSlotFloats, 8 kSymratePiece, 9 kSymrateHalo, 10 kSymrateThreads, 11 kSymrateMinS, 12 kSymrateMaxS, 13 kSymrateMaxBlocks,
// 14 kAcquirePiece, 15 kAcquireHalo, 16 kAcquireThreads, 17 kSyncPiece, 18 kSyncThreads, 19 kSyncHist, 20 kSyncHistSlotFloats,
// 21 kSyncMaxWord, 22 kSyncHits
int psk_prepass_probe_constant(int which)
{
    switch (which) {
    case 0: return (int)kResamplePiece;
    case 1: return (int)kResampleInputs;
    case 2: return (int)kGatherTile;
    case 3: return (int)kGatherMinGroup;
    case 4: return (int)kTuneTableFloats;
    case 5: return (int)kFirWindow;
    case 6: return (int)kFirMaxTaps;
    case 7: return (int)kFirHistSlotFloats;
    case 8: return (int)kSymratePiece;
    case 9: return (int)kSymrateHalo;
    case 10: return (int)kSymrateThreads;
    case 11: return (int)kSymrateMinS;
    case 12: return (int)kSymrateMaxS;
    case 13: return (int)kSymrateMaxBlocks;
    case 14: return (int)kAcquirePiece;
    case 15: return (int)kAcquireHalo;
    case 16: return (int)kAcquireThreads;
    case 17: return (int)kSyncPiece;
    case 18: return (int)kSyncThreads;
    case 19: return (int)kSyncHist;
    case 20: return (int)kSyncHistSlotFloats;
    case 21: return (int)kSyncMaxWord;
    case 22: return (int)kSyncHits;
    default: return -1;
    }
}

// fir_piece(decim): outputs of one piece of the filter pass at that decimation; -1 outside 1 .. kFirMaxDecim
int psk_prepass_probe_fir_piece(int decim)
{
    return decim >= 1 && decim <= (int)kFirMaxDecim ? (int)fir_piece((uint32_t)decim) : -1;
}

int psk_prepass_probe_gather_singles(void *arena, uint64_t bytes, int sample_bytes, const void *desc, uint32_t n_desc, uint64_t max_n)
{
    if (!arena || !bytes || !desc || !n_desc)
        return (int)hipErrorInvalidValue;
    std::vector<GatherSingle> d((const GatherSingle *)desc, (const GatherSingle *)desc + n_desc);
    Run r;
    if (!r.begin(arena, bytes))
        return r.end(hipSuccess, arena, 0, nullptr);
    for (GatherSingle &s : d)
        if (!point(s.src, r.d_arena, bytes) || !point(s.dst, r.d_arena, bytes))
            return r.end(hipErrorInvalidValue, arena, 0, nullptr);
    if (!r.descriptors(0, d.data(), sizeof(GatherSingle) * d.size()))
        return r.end(hipSuccess, arena, 0, nullptr);
    return r.end(launch_gather_singles(sample_bytes, (const GatherSingle *)r.d_desc[0], n_desc, max_n, r.stream), arena, bytes, nullptr);
}

int psk_prepass_probe_gather_tiles(void *arena, uint64_t bytes, int sample_bytes, const void *groups, uint32_t n_groups, const void *chans,
                                   uint32_t n_chans, uint64_t n_tiles)
{
    if (!arena || !bytes || !groups || !n_groups || !chans || !n_chans)
        return (int)hipErrorInvalidValue;
    std::vector<GatherGroup> g((const GatherGroup *)groups, (const GatherGroup *)groups + n_groups);
    std::vector<GatherChan> c((const GatherChan *)chans, (const GatherChan *)chans + n_chans);
    Run r;
    if (!r.begin(arena, bytes))
        return r.end(hipSuccess, arena, 0, nullptr);
    for (GatherGroup &x : g)
        if (!point(x.src, r.d_arena, bytes) || (uint64_t)x.first + x.g > n_chans)
            return r.end(hipErrorInvalidValue, arena, 0, nullptr);
    for (GatherChan &x : c)
        if (!point(x.dst, r.d_arena, bytes))
            return r.end(hipErrorInvalidValue, arena, 0, nullptr);
    if (!r.descriptors(0, g.data(), sizeof(GatherGroup) * g.size()) || !r.descriptors(1, c.data(), sizeof(GatherChan) * c.size()))
        return r.end(hipSuccess, arena, 0, nullptr);
    return r.end(launch_gather_tiles(sample_bytes, (const GatherGroup *)r.d_desc[0], n_groups, (const GatherChan *)r.d_desc[1], n_tiles, r.stream),
                 arena, bytes, nullptr);
}

// tables_out: kTuneTableFloats floats, the device's copy of tune_tables() as it is behind the launch
int psk_prepass_probe_tune(void *arena, uint64_t bytes, const void *desc, uint32_t n_desc, uint64_t max_n, float *tables_out)
{
    if (!arena || !bytes || !desc || !n_desc)
        return (int)hipErrorInvalidValue;
    std::vector<TuneDesc> d((const TuneDesc *)desc, (const TuneDesc *)desc + n_desc);
    Run r;
    if (!r.begin(arena, bytes))
        return r.end(hipSuccess, arena, 0, nullptr);
    for (TuneDesc &t : d)
        if (!point(t.src, r.d_arena, bytes) || !point(t.dst, r.d_arena, bytes))
            return r.end(hipErrorInvalidValue, arena, 0, nullptr);
    if (!r.descriptors(0, d.data(), sizeof(TuneDesc) * d.size()) || !r.tables())
        return r.end(hipSuccess, arena, 0, nullptr);
    return r.end(launch_tune((const TuneDesc *)r.d_desc[0], n_desc, max_n, r.d_tab, r.stream), arena, bytes, tables_out);
}

int psk_prepass_probe_resample(void *arena, uint64_t bytes, const void *desc, uint32_t n_desc, uint64_t max_n_out)
{
    if (!arena || !bytes || !desc || !n_desc)
        return (int)hipErrorInvalidValue;
    std::vector<ResampleDesc> d((const ResampleDesc *)desc, (const ResampleDesc *)desc + n_desc);
    Run r;
    if (!r.begin(arena, bytes))
        return r.end(hipSuccess, arena, 0, nullptr);
    for (ResampleDesc &t : d)
        if (!point(t.io.src, r.d_arena, bytes) || !point(t.io.dst, r.d_arena, bytes) || !point(t.hist_in, r.d_arena, bytes) ||
            !point(t.hist_out, r.d_arena, bytes))
            return r.end(hipErrorInvalidValue, arena, 0, nullptr);
    if (!r.descriptors(0, d.data(), sizeof(ResampleDesc) * d.size()) || !r.tables())
        return r.end(hipSuccess, arena, 0, nullptr);
    return r.end(launch_resample((const ResampleDesc *)r.d_desc[0], n_desc, max_n_out, r.d_tab, r.stream), arena, bytes, nullptr);
}

// max_pieces: the most pieces (of fir_piece(decim) outputs) any packet of the launch has
int psk_prepass_probe_fir(void *arena, uint64_t bytes, const void *desc, uint32_t n_desc, uint64_t max_pieces)
{
    if (!arena || !bytes || !desc || !n_desc)
        return (int)hipErrorInvalidValue;
    std::vector<FirDesc> d((const FirDesc *)desc, (const FirDesc *)desc + n_desc);
    Run r;
    if (!r.begin(arena, bytes))
        return r.end(hipSuccess, arena, 0, nullptr);
    for (FirDesc &t : d)
        if (!point(t.io.src, r.d_arena, bytes) || !point(t.io.dst, r.d_arena, bytes) || !point(t.taps, r.d_arena, bytes) ||
            !point(t.hist_in, r.d_arena, bytes) || !point(t.hist_out, r.d_arena, bytes))
            return r.end(hipErrorInvalidValue, arena, 0, nullptr);
    if (!r.descriptors(0, d.data(), sizeof(FirDesc) * d.size()) || !r.tables())
        return r.end(hipSuccess, arena, 0, nullptr);
    return r.end(launch_fir((const FirDesc *)r.d_desc[0], n_desc, max_pieces, r.d_tab, r.stream), arena, bytes, nullptr);
}

// The two looks: fold, then join, one launch each.  part_off, rec_off: where the partials (slot 0) and the records (channel 0) lie
// in the arena; a descriptor without its DATA flag keeps the null source the product gives it.
int psk_prepass_probe_symrate(void *arena, uint64_t bytes, const void *desc, uint32_t n_desc, uint32_t max_piece, uint64_t part_off,
                              uint64_t rec_off)
{
    if (!arena || !bytes || !desc || !n_desc || part_off >= bytes || rec_off >= bytes || part_off % 8u || rec_off % 8u)
        return (int)hipErrorInvalidValue;
    std::vector<SymrateDesc> d((const SymrateDesc *)desc, (const SymrateDesc *)desc + n_desc);
    Run r;
    if (!r.begin(arena, bytes))
        return r.end(hipSuccess, arena, 0, nullptr);
    for (SymrateDesc &t : d)
        if ((t.flags & PSK_SOFT_SR_DATA) && !point(t.src, r.d_arena, bytes))
            return r.end(hipErrorInvalidValue, arena, 0, nullptr);
    if (!r.descriptors(0, d.data(), sizeof(SymrateDesc) * d.size()) || !r.tables())
        return r.end(hipSuccess, arena, 0, nullptr);
    SymratePartial *const part = (SymratePartial *)(r.d_arena + part_off);
    hipError_t e = launch_symrate_fold((const SymrateDesc *)r.d_desc[0], n_desc, max_piece, r.d_tab, part, r.stream);
    if (e == hipSuccess)
        e = launch_symrate_join((const SymrateDesc *)r.d_desc[0], n_desc, part, (psk_soft_symrate_t *)(r.d_arena + rec_off), r.stream);
    return r.end(e, arena, bytes, nullptr);
}

// with_tables 0: the launch has no tuned packet, the fold gets no tables (psk_acquire_fold_kernel<false>)
int psk_prepass_probe_acquire(void *arena, uint64_t bytes, const void *desc, uint32_t n_desc, uint32_t max_piece, uint64_t part_off,
                              uint64_t rec_off, int with_tables)
{
    if (!arena || !bytes || !desc || !n_desc || part_off >= bytes || rec_off >= bytes || part_off % 8u || rec_off % 8u)
        return (int)hipErrorInvalidValue;
    std::vector<AcquireDesc> d((const AcquireDesc *)desc, (const AcquireDesc *)desc + n_desc);
    Run r;
    if (!r.begin(arena, bytes))
        return r.end(hipSuccess, arena, 0, nullptr);
    for (AcquireDesc &t : d)
        if (((t.flags & PSK_SOFT_A_DATA) && !point(t.src, r.d_arena, bytes)) || ((t.flags & PSK_SOFT_A_TUNED) && !with_tables))
            return r.end(hipErrorInvalidValue, arena, 0, nullptr);
    if (!r.descriptors(0, d.data(), sizeof(AcquireDesc) * d.size()) || (with_tables && !r.tables()))
        return r.end(hipSuccess, arena, 0, nullptr);
    AcquirePartial *const part = (AcquirePartial *)(r.d_arena + part_off);
    hipError_t e = launch_acquire_fold((const AcquireDesc *)r.d_desc[0], n_desc, max_piece, r.d_tab, part, r.stream);
    if (e == hipSuccess)
        e = launch_acquire_join((const AcquireDesc *)r.d_desc[0], n_desc, part, (psk_soft_acquire_t *)(r.d_arena + rec_off), r.stream);
    return r.end(e, arena, bytes, nullptr);
}

// The word search: which bit 0 launches the fold, bit 1 the join, on one stream in that order.  soft, word, hist_in and hist_out of
// a descriptor with kSyncData are arena offsets; a descriptor without it is passed as it is.
int psk_prepass_probe_sync(void *arena, uint64_t bytes, const void *desc, uint32_t n_desc, uint32_t max_piece, uint64_t part_off,
                           uint64_t rec_off, int which)
{
    if (!arena || !bytes || !desc || !n_desc || part_off >= bytes || rec_off >= bytes || part_off % 8u || rec_off % 8u || !(which & 3) ||
        (which & ~3))
        return (int)hipErrorInvalidValue;
    std::vector<SyncDesc> d((const SyncDesc *)desc, (const SyncDesc *)desc + n_desc);
    Run r;
    if (!r.begin(arena, bytes))
        return r.end(hipSuccess, arena, 0, nullptr);
    for (SyncDesc &t : d)
        if ((t.flags & kSyncData) && (!point(t.soft, r.d_arena, bytes) || !point(t.word, r.d_arena, bytes) ||
                                      !point(t.hist_in, r.d_arena, bytes) || !point(t.hist_out, r.d_arena, bytes)))
            return r.end(hipErrorInvalidValue, arena, 0, nullptr);
    if (!r.descriptors(0, d.data(), sizeof(SyncDesc) * d.size()))
        return r.end(hipSuccess, arena, 0, nullptr);
    SyncPartial *const part = (SyncPartial *)(r.d_arena + part_off);
    hipError_t e = hipSuccess;
    if (which & 1)
        e = launch_sync_fold((const SyncDesc *)r.d_desc[0], n_desc, max_piece, part, r.stream);
    if (e == hipSuccess && (which & 2))
        e = launch_sync_join((const SyncDesc *)r.d_desc[0], n_desc, part, (psk_soft_sync_t *)(r.d_arena + rec_off), r.stream);
    return r.end(e, arena, bytes, nullptr);
}

}  // extern "C"
