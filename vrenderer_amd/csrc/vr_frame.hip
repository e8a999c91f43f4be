// vr_frame_submit: one frame of the hot path as ONE call - the terrain part of Renderer::RecordCommand (Renderer.cpp:321-446:
// one command list per frame): Clear (fused, assume_cleared) -> TerrainPass::Render (:401-415) -> DeferredLightingPass::Render
// (:417-428) -> ToneMappingPass::SimpleRender (:430-431) [-> the N-rank exchange], plus the geometry of up to two upcoming
// frames built ahead (vr_terrain_prepare).  It queues exactly what the per-call entry points queue, in the same order on the
// same streams; what it removes is the host's per-call cost - a frame is about nine calls otherwise, and a rank of an 8-way
// split of the 8K frame has a period near 0.1 ms (the host needed 98 us per frame through the Python wrappers).
// The cross-stream order between the lighting pass (terrain's context) and a tone-map stage on another context's stream is
// the library's here: the stage waits for the lighting pass's stop event, and an image remembers who still reads it, so a
// later lighting pass into the same vr_image waits for that reader (a host that rotates two images keeps both streams busy).
// The frame refuses before it queues anything: the lighting pass's arguments (vr_light_check), the tone-map stage's - sizes
// and capacities included -, the exchange's, the LDR de-tile's width and the RCCL entry points (vr_tonemap_stage, queue = false)
// are all looked at in front of the tile pass.  A refused frame leaves the G-buffer, its pending clear, HdrColor, the bins and
// the adapted luminance as they were, and a rank of an N-GPU run never enters one collective and skips the next.  What is left
// behind the tile pass is what that pass itself refuses (its own arguments) and what a HIP call reports.
#include "vr_deferred_dev.h"

extern "C" VR_API int vr_frame_submit(vr_terrain* t, vr_gbuffer* gb, const vr_frame_desc* f)
{
    VR_REQUIRE(t && gb && f && f->view && f->render && f->hdr_out, "NULL argument");
    VR_REQUIRE(f->num_lights >= 0 && (f->num_lights == 0 || f->lights), "lights is NULL");
    vr_context* ctx = t->ctx;
    VR_REQUIRE(gb->ctx == ctx && f->hdr_out->ctx->device == ctx->device, "G-buffer / image belong to another context");
    vr_image* hdr = f->hdr_out;
    int rc;
    // tiled: 2 = every light type and the shadow binding (vr_deferred_light_tiled_ex); any other non-zero value = 1 =
    // vr_deferred_light_tiled, which has no shadow term: the binding is ignored
    const LightEntry entry = f->tiled == 2 ? LIGHT_TILED_EX : f->tiled ? LIGHT_TILED : LIGHT_STREAM;
    LightCall lc;
    if ((rc = vr_light_check(ctx, entry, f->view, gb, f->lights, f->num_lights, f->ambient_top, f->ambient_bottom, hdr, f->part, f->shadow, &lc))) return rc;
    // ToneMappingPass::SimpleRender [+ the bins' all-reduce] on the tone mapper's own context
    TmStageCall tmc{};
    if (f->tonemap) {
        tmc.steps = TM_RESET | TM_HISTOGRAM | (f->nccl_comm ? TM_ALLREDUCE : 0u) | TM_EXPOSURE | TM_RENDER;
        tmc.p = f->tonemap_params; tmc.frame_time = f->frame_time_seconds; tmc.hdr = hdr; tmc.w = gb->w; tmc.h = gb->h;
        tmc.ldr = f->ldr_out; tmc.ldr_capacity = f->ldr_capacity; tmc.part = f->part; tmc.comm = f->nccl_comm; tmc.frame = f; tmc.frame_device = ctx->device;
        if ((rc = vr_tonemap_stage(f->tonemap, tmc, false))) return rc;
    }
    // TerrainPass::Render, then the chains of the next frames under its tile pass (a frame already prepared is a no-op)
    // (a sticky code - VR_ERR_TOO_MANY_INSTANCES / VR_ERR_OVERFLOW of an EARLIER frame - does not stop this one: it is returned at the end)
    // Under VR_OPT_FRAME_FUSION the tile pass shades as well where its G-buffer-keeping flavour applies (the plain streaming
    // lighting pass of a whole frame; everything else is decided in vr_terrain_render_keep, in front of the launch): the frame is
    // then one kernel, and what the G-buffer, its plane states and HdrColor hold afterwards is what the two passes leave.
    // Outside sky_is_zero (vr_light_domain.h) nothing fuses: the resolve would store +0 for a sky pixel that the model does not
    // shade to +0 there, so the frame is the unfused pair, whose lighting pass is then k_deferred_stream (vr_light_plan.h).
    bool fused = false;
    VrEventRef fused_stop;
    int earlier;
    if (ctx->frame_fusion && !f->tiled && !f->shadow && !f->part)
        earlier = vr_terrain_render_keep(t, f->view, gb, f->render, f->lights, f->num_lights, f->ambient_top, f->ambient_bottom, hdr, !lc.in.sky_not_zero, &fused, &fused_stop);
    else earlier = vr_terrain_render(t, f->view, f->view, gb, f->render, f->part);
    if (earlier != VR_OK && earlier != VR_ERR_TOO_MANY_INSTANCES && earlier != VR_ERR_OVERFLOW) return earlier;
    for (int k = 0; k < 2; k++)
        if (f->prepare_views[k] && (rc = vr_terrain_prepare(t, f->prepare_views[k], gb, f->render, f->part))) return rc;
    // whoever still reads the image this lighting pass overwrites (the tone-map stage of two frames ago, on another stream)
    // (a fused tile pass has waited for that reader in front of its own launch)
    // written_stop: the stop event of the pass that writes the image - the fused tile pass's or the lighting pass's OWN, handed out
    // by the launch (vr_terrain_prepare has run since: the context's last stamped launch need not be that one)
    const VrOrderOps ops;
    VrEventRef written_stop = fused_stop;
    if (!fused) {
        if ((rc = order_image_writer_begins(hdr->ord, ops, ctx->stream))) return rc;
        if ((rc = vr_light_queue(ctx, gb, hdr, f->part, f->shadow, lc, &written_stop))) return rc;
    }
    if (!f->tonemap) return earlier;

    // the tone-map stage (another stream: it runs under the next frame's rendering)
    vr_context* tc = vr_tonemap_context(f->tonemap);
    const bool cross = tc->stream != ctx->stream;
    if (cross) {
        // behind the pass that wrote the image: its dispatch-stamped stop event when there is one, else an explicit record
        if (!written_stop.ev && !hdr->ord.written.own) VR_HIP(hipEventCreateWithFlags(&hdr->ord.written.own, hipEventDisableTiming));
        if ((rc = order_image_written(hdr->ord, ops, ctx->stream, tc->stream, written_stop, ctx->events))) return rc;
    }
    if ((rc = vr_tonemap_stage(f->tonemap, tmc, true))) return rc;
    if (cross) {
        if (!hdr->ord.read_done.ev) VR_HIP(hipEventCreateWithFlags(&hdr->ord.read_done.ev, hipEventDisableTiming));
        if ((rc = order_image_reader_done(hdr->ord, ops, tc->stream))) return rc;
    }
    if (f->nccl_comm && (rc = vr_frame_allgather_ldr(tc, f->nccl_comm, f->ldr_out, f->gathered, f->part->world_size, gb->w, gb->h, f->ldr_frame))) return rc;
    return earlier;
}
