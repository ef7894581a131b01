// The transitions of pep_ctx::side[] / pep_ctx::holds (common.h), the only code that assigns them; each also drops what was derived from the sets it touches:
// nucl_valid, t_class_ready / group_of_seq, k1_base_frames, self_first_n.  Which call makes which transition: DESIGN.md section 3.1.
#pragma once
#include "common.h"
// one side is not packed (any more); the reference side's self-search map goes with its packing (K1 writes it again)
inline void side_unpacked(pep_ctx *ctx, PepSide s) { ctx->side[s].packed = Packed::No; if (s == PEP_SIDE_T) ctx->self_first_n = 0; }
// pep_set_query_nt / pep_set_ref_nt (frames: reference side only)
inline void sets_given_nt(pep_ctx *ctx, PepSide s, int gtable, int frames = 0)
{
    ctx->side[s].source = SetSource::Nt; ctx->side[s].gtable = gtable;
    side_unpacked(ctx, s);
    ctx->holds = SetsHold::Inputs;
    ctx->nucl_valid = false;
    if (s == PEP_SIDE_T) { ctx->side[s].frames = frames; ctx->k1_base_frames = 0; ctx->group_of_seq.clear(); ctx->t_class_ready = false; }
}
// a side's host tables (meta records, h_off, h_len) are there: upload_aa, pep_k1_host_tables
inline void side_tables_built(pep_ctx *ctx, PepSide s) { ctx->side[s].tables_built = true; }
// pep_set_query_aa / pep_set_ref_aa, behind the upload
inline void sets_given_residues(pep_ctx *ctx, PepSide s)
{
    ctx->side[s].source = SetSource::Residues; ctx->side[s].packed = Packed::Yes;
    ctx->holds = SetsHold::Inputs;
    if (s == PEP_SIDE_T) { ctx->self_first_n = 0; ctx->group_of_seq.clear(); ctx->t_class_ready = false; }
}
// pep_set_target_groups with other contents than the ones in force (the nucleotide tool's targets are laid out group by group)
inline void sets_groups_changed(pep_ctx *ctx, const uint32_t *group, uint32_t n)
{
    ctx->group_of_seq.assign(group, group + n);
    ctx->t_class_ready = false; ctx->nucl_valid = false;
}
// K1 of a side is on the stream / its summary has been taken (the host tables wait on the device)
inline void side_queued(pep_ctx *ctx, PepSide s) { ctx->side[s].packed = Packed::Queued; }
inline void side_taken(pep_ctx *ctx, PepSide s) { ctx->side[s].packed = Packed::Yes; ctx->side[s].tables_built = false; }
// a failure while a side was queued: it is not packed, the next search translates again
struct DropQueuedOnExit { pep_ctx *ctx; ~DropQueuedOnExit() { for (PepSide s : {PEP_SIDE_Q, PEP_SIDE_T}) if (ctx->side[s].packed == Packed::Queued) side_unpacked(ctx, s); } };
inline void sets_invalidate_translation(pep_ctx *ctx) { for (PepSide s : {PEP_SIDE_Q, PEP_SIDE_T}) if (ctx->side[s].from_nt()) side_unpacked(ctx, s); }
// What ctx->q / ctx->t hold changes.  Inputs: pep_translate, K1 - whatever K1 is about to do, the sets no longer count as the nucleotide tool's.  TakenOver: somebody
// else writes them from here on (the gapped stage of pep_linclust; pep_use_nt_as_residues until its sets are complete) - a later search needs K1 or, for residue
// sources, its inputs again.  BaseCodes: pep_nucl_sets has made both sets, and their host tables, from the kept layouts
inline void sets_hold(pep_ctx *ctx, SetsHold h)
{
    ctx->holds = h;
    if (h == SetsHold::TakenOver) { side_unpacked(ctx, PEP_SIDE_Q); side_unpacked(ctx, PEP_SIDE_T); ctx->t_class_ready = false; }
    if (h == SetsHold::BaseCodes) { side_tables_built(ctx, PEP_SIDE_Q); side_tables_built(ctx, PEP_SIDE_T); }
}
