"""The pretraining loop of the reference (train.py:120-296) around the HIP train step: same flags, same per-iteration order
(zero_grad -> batch -> forward -> backward -> clip_grad_norm -> optimizer step -> scaler update -> scheduler step), same
logging / checkpoint / validation cadence. Differences, all forced by the target: the gradient mean over ranks is an explicit
RCCL exchange of the flat gradient arena overlapped with backward (utils/distributed.py) instead of DistributedDataParallel;
clipping + SGD + Lookahead run in one fused kernel; wandb/loguru (absent from the image) are replaced by the stdlib logger."""
import argparse
import contextlib
import os
from collections import Counter
from typing import Any

import torch
from torch.utils.data import DataLoader, DistributedSampler

from .config import Config
from .factories import LRSchedulerFactory, NegativeSamplingDatasetFactory, OptimizerFactory, PretrainingDatasetFactory, PretrainingModelFactory
from .utils import distributed as dist
from .utils.base import Timer, make_directory
from .utils.checkpointing import CheckpointManager
from .utils.common import GradScaler, common_parser, common_setup, cycle, logger


def build_parser():
    parser = common_parser(description="Train the VLInfo (CLIP-Lite) model on image-caption pairs.")
    group = parser.add_argument_group("Checkpointing and Logging")
    group.add_argument("--resume-from", default=None, help="Path to a checkpoint to resume training from (if provided).")
    group.add_argument("--checkpoint-every", type=int, default=10000, help="Serialize model to a checkpoint after every these many iterations.")
    group.add_argument("--log-every", type=int, default=500, help="Log training curves after every these many iterations.")
    group.add_argument("--climax-freq", type=int, default=1000, help="Frequency to checkpoint at during climax (last 20%% training)")
    group = parser.add_argument_group("MI355X launch path (not in the reference)")
    group.add_argument("--allow-eager-fallback", action="store_true", help="If the hipGraph capture of the step fails, log an error and continue with "
                       "eager launches instead of stopping.")
    group.add_argument("--grad-exchange", default="allreduce", choices=["allreduce", "mesh"], help="Gradient mean over ranks: one RCCL all-reduce per "
                       "region, or the direct mesh form (all-to-all, local sum, all-gather) for a fully connected xGMI node.")
    group.add_argument("--no-hip-graph", action="store_true", help="Launch every kernel of the step from Python instead of replaying the "
                       "captured hipGraphs of the step (TrainStep graph mode; batches of another shape always take the eager path).")
    return parser


def check_cluster_assets(_C):
    """With "clusters" in DATA.NEGATIVE_SAMPLING the cluster maps must exist when the run starts, also when the switch lies in the future: a run
    must not die at iteration NEGATIVE_SAMPLING_START_ITERATION."""
    from .data import get_cluster_options
    path = _C.DATA.CLUSTER_PATH
    try:
        options = get_cluster_options(path, "train")
    except FileNotFoundError:
        options = []
    if not options:
        raise FileNotFoundError(f"DATA.NEGATIVE_SAMPLING {_C.DATA.NEGATIVE_SAMPLING!r} needs img_id_cluster_map_train_<k>.pkl files in DATA.CLUSTER_PATH "
                                f"({path!r}), and there are none: write them with cluster.py (python cluster.py --config ... --cluster-root ...)")
    return options


def init_dataloaders(_C, _A, type="normal"):
    """reference train.py:60-118. type "clusters": the clustered datasets at half the per-rank batch (train.py:75: the step then encodes B / 2
    pairs and B / 2 negatives)."""
    if type == "normal":
        train_dataset = PretrainingDatasetFactory.from_config(_C, split="train")
        val_dataset = PretrainingDatasetFactory.from_config(_C, split="val")
        batch_size = _C.OPTIM.BATCH_SIZE // dist.get_world_size()
    elif type == "clusters":
        from .data import get_cluster_options
        check_cluster_assets(_C)
        train_dataset = NegativeSamplingDatasetFactory.from_config(_C, split="train")
        if get_cluster_options(_C.DATA.CLUSTER_PATH, "val"):
            val_dataset = NegativeSamplingDatasetFactory.from_config(_C, split="val")
        else:
            logger.warning(f"no img_id_cluster_map_val_<k>.pkl in {_C.DATA.CLUSTER_PATH!r}: validating on the normal val dataset (no negatives)")
            val_dataset = PretrainingDatasetFactory.from_config(_C, split="val")
        batch_size = (_C.OPTIM.BATCH_SIZE // dist.get_world_size()) // 2
    else:
        raise KeyError(f"init_dataloaders: unknown type {type!r} (normal | clusters)")
    distributed = dist.get_world_size() > 1
    train_sampler = DistributedSampler(train_dataset, shuffle=True) if distributed else None
    val_sampler = DistributedSampler(val_dataset, shuffle=False) if distributed else None
    train_dataloader = DataLoader(train_dataset, batch_size=batch_size, sampler=train_sampler, shuffle=train_sampler is None,
                                  num_workers=_A.cpu_workers, pin_memory=True, drop_last=True, collate_fn=train_dataset.collate_fn)
    val_dataloader = DataLoader(val_dataset, batch_size=batch_size, sampler=val_sampler, shuffle=False, num_workers=_A.cpu_workers,
                                pin_memory=True, drop_last=False, collate_fn=val_dataset.collate_fn)
    return train_dataloader, val_dataloader


class TrainStep:
    """One optimisation step on one rank: reference train.py:211-226.

    `graph=True` records the step (forward, backward, squared gradient norm, fused clip + SGD + Lookahead update: ~900 kernel
    launches) into hipGraphs after `graph_warmup` eager steps and replays them afterwards, which takes the Python/launch cost off
    the critical path. What changes per step is fed from the host before each replay: the batch (copied into the captured input
    buffers), the update kernel's hyper-parameters (LR schedule value, Lookahead sync flag) and, on the device, the dropout seeds
    (runtime.DeviceRuntime.sync_graph_seeds). Eager and replayed steps run the same kernels on the same arguments.

    Data parallel (`exchange` given): the step is recorded as two graphs — [forward + backward] and [gradient norm + update] —
    with the RCCL all-reduce of the flat gradient arena issued eagerly between them (collectives stay outside the captures)."""

    def __init__(self, model, optimizer, scheduler, scaler, clip_grad_norm, exchange=None, graph=False, graph_warmup=2, pad_to=None,
                 allow_eager_fallback=False, defer_update=False):
        """pad_to: caption length the step is captured at (DATA.MAX_CAPTION_LENGTH). The reference's collate pads each batch to ITS longest
        caption (data/dataloader.py:218-236), so L changes from batch to batch; shorter batches are right-padded (id 0 = [PAD], mask 0) into
        the captured buffers. Masked positions receive exactly zero attention weight and feed nothing downstream of the [CLS] pooler, so
        features, loss and gradients are those of the unpadded batch. allow_eager_fallback: continue with eager launches if the capture
        fails (default: raise — an eager step pays ~20 ms of Python launches, several times the replay at small batches)."""
        self.model, self.optimizer, self.scheduler, self.scaler = model, optimizer, scheduler, scaler
        self.pad_to, self.allow_eager_fallback = pad_to, allow_eager_fallback
        self.clip, self.exchange = clip_grad_norm, exchange
        self.inner = optimizer.optimizer if hasattr(optimizer, "optimizer") else optimizer
        self.graph = bool(graph)
        # defer_update (captured per-phase steps only): the update needs the global gradient norm, i.e. the LAST weight gradient of the image
        # backward, so it cannot start earlier — but only the image encoder's parameters are needed right away (the next image forward). With
        # defer_update the step ends after [norm + update of the image encoder]; the text encoder's and the heads' share (85 % of the parameters,
        # 0.7 of the 0.87 ms) runs as the FIRST thing of the next step on the text encoder's stream, which idles ~1 ms there while the image
        # forward is still going. Same kernels, same arguments, every tensor updated exactly once per step: parameters are bit-identical to the
        # undeferred step once finish() has run. Anything that reads parameters between steps (checkpoint, evaluation, state_dict) completes it
        # first: Arena.flush_pending (state_dict / load_state_dict / refresh_lowp / eval forward call it), train_loop.main and bench.py call
        # finish(). Round 3 measured it neutral (17.32 vs 17.35 ms); with round 4's shorter side stream it gains 0.1 ms (15.14 -> 15.04, same box):
        # train_loop.main and bench.py switch it on; the constructor default stays off (tests build TrainStep directly).
        self.defer_update = bool(defer_update)
        self._pending_rest = False
        self._rest_ev = None           # recorded on the side stream behind a deferred update_rest replay; the main stream waits on it before the heads
        if self.defer_update:          # readers of the parameters outside the step complete the update first (Arena.flush_pending)
            self.inner.arena.pending_update = self.finish
        self.graph_warmup = graph_warmup
        self._eager_steps = 0
        self._g = self._g_update = self._graphs = None
        self._static_batch = self._static_out = None
        self.replays = self.eager_steps = 0        # how many steps took the captured / the eager launch path

    def finish(self):
        """Run what a deferred step left undone (the update of everything but the image encoder); no-op otherwise. Leaves the current stream
        ordered behind it."""
        if not self._pending_rest:
            return
        rt = self.model.runtime
        main, side = torch.cuda.current_stream(rt.device), rt.side_stream
        side.wait_stream(main)
        with torch.cuda.stream(side):
            self._graphs["update_rest"].replay()
        main.wait_stream(side)
        self._pending_rest = False
        self._rest_ev = None

    def recapture(self):
        """Forget the captured step: complete a deferred update, drop the graphs and their static buffers, and let the next calls warm up and
        capture again on the batches that arrive then. train_loop.main calls it when the loader switches to clustered negative sampling: those
        batches (new neg_* keys, half the rows) do not fit the captured graphs, and every later step would silently take the eager path."""
        self.finish()
        torch.cuda.synchronize()
        self._g = self._g_update = self._graphs = None
        self._static_batch = self._static_out = None
        self._keep = self._staged = None
        self._eager_steps = 0

    def _eager(self, batch):
        # (another TrainStep on the same model may hold the pending share: Arena.flush_pending reaches whichever one registered last — ADVICE r4)
        self.finish()
        self.inner.arena.flush_pending()
        self.eager_steps += 1
        self.optimizer.zero_grad()
        output_dict = self.model(batch)
        loss = output_dict["loss"]
        self.scaler.scale(loss).backward()
        if self.exchange is not None:
            self.inner.grad_prescale = self.exchange.finish()       # wait for the gradient mean (SUM here, 1/world in the update)
        self.scaler.unscale_(self.optimizer)
        if self.clip and self.clip > 0:
            self.optimizer.clip_grad_norm(self.clip)
        self.scaler.step(self.optimizer)
        self.scaler.update()
        self.scheduler.step()
        return output_dict

    def _capture_update(self):
        self.inner.arena.join()
        if self.clip and self.clip > 0:
            self.inner._build_items()
            self.inner.zero_frozen()          # frozen tensors' unconditional gradients must not enter the norm
            self.inner.sumsq.zero_()
            hip_sumsq(self.inner)
        self.inner.launch()

    # ---- captured step ------------------------------------------------------------------------------------------------
    # One hipGraph per phase, replayed on two HIP streams: HIP executes the nodes of a single captured graph almost serially
    # (measured: 84 % of a one-graph step had exactly one kernel in flight), so real concurrency between the two encoders needs
    # separate graphs on separate streams:
    #
    #   main : [image fwd] ------------> [heads fwd + bwd] --> [image bwd chain: layer4,3 | layer2 | layer1,stem] [wgrads 1,stem] --> [norm + update]
    #   side : [text  fwd] --(join)--^          (fork)-----> [text  bwd + its grouped wgrads] [wgrads 4,3] [wgrads 2] ---------(join)--^
    #   comm :                                     all-reduce(heads)                     all-reduce(text)  all-reduce(image)     (data parallel)
    #
    # Graphs that replay on the same stream share a memory pool (they run in capture order); the two streams use different pools,
    # and every tensor that crosses a stream (features, their gradients) is kept referenced for the lifetime of the graphs.
    def _direct_ok(self):
        m = self.model
        inert = self._inert_params()
        from .loss import GlobalDiscriminatorDot
        from .resnet import ResNet
        # (the per-phase graphs are scheduled around the ResNet's backward segments and BERT's: a ViT image encoder, and the CLIP text tower
        # whatever the image encoder is, take the whole step as one graph)
        return (getattr(m, "mode", None) == "train_sbert" and not m.text_encoder.transform_embedding and m.training
                and getattr(getattr(m.text_encoder, "strans", None), "kind", "bert") != "clip"
                and isinstance(getattr(m.image_encoder, "img_encoder", None), ResNet)
                and isinstance(m.loss.global_d, GlobalDiscriminatorDot)
                and not getattr(m.image_encoder, "frozen", False)
                and all(p.requires_grad for p in m.parameters() if id(p) not in inert))

    def _inert_params(self):
        """Parameters that exist for checkpoint-key parity only and are frozen by construction (the MPNet tower's pooler, mpnet.py): they do not make
        the model a partly frozen one for the per-phase capture."""
        st = getattr(self.model.text_encoder, "strans", None)
        return {id(p) for p in st.pooler.parameters()} if getattr(st, "kind", "bert") == "mpnet" else set()

    def _capture(self, batch):
        if not self._direct_ok() or any(k in batch for k in ("neg_input_ids", "aug_image", "aug_image_plan", "aug_input_ids")):
            return self._capture_single(batch)
        from .bert import bert_backward, bert_forward
        from .loss import jsd_backward, jsd_forward
        from .resnet import resnet_backward, resnet_forward
        m, rt = self.model, self.model.runtime
        sb = self._static_batch = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in self._padded(batch).items()}
        self.optimizer.zero_grad()            # no-op after a completed step (the update kernel leaves the gradients zeroed)
        torch.cuda.synchronize()
        saved_exchange, rt.exchange = rt.exchange, None      # the executors must not start collectives inside a capture
        pool_main, pool_side = torch.cuda.graph_pool_handle(), torch.cuda.graph_pool_handle()
        graphs, keep = {}, {}

        # other threads keep making HIP calls of their own during a capture — RCCL's watchdog / proxy threads in data parallel, the
        # DataLoader's pin-memory thread in any real run (a capture in "global" mode is invalidated by them: hipErrorStreamCaptureInvalidated);
        # only this thread's calls belong to the capture
        mode = "thread_local"

        dump_dir = getattr(self, "debug_graph_dir", None)          # tools/graph_nodes.py: the node list of every captured phase (hipGraphDebugDotPrint)

        def capture(name, pool, fn):
            rt._zpools = {}                   # a segment zeroes the accumulators it uses itself
            g = torch.cuda.CUDAGraph()
            if dump_dir:
                g.enable_debug_mode()
            with torch.cuda.graph(g, pool=pool, capture_error_mode=mode):
                fn()
            if dump_dir:
                g.debug_dump(os.path.join(dump_dir, name + ".dot"))
            graphs[name] = g

        # the image is staged (NCHW f32 -> padded NHWC4, one kernel) OUTSIDE the graphs, straight from the caller's tensor into the buffer the
        # captured stem reads: a replay then never copies the 77 MB batch into a static input first
        if "image_u8" in sb:
            # a batch of the GPU-augmenting loader (DATA.GPU_AUGMENT): the augmentation kernels write the views of the caller's canvases
            # straight into that buffer (augment.stage_views: a gray pass for the jittered views, then one launch) - no f32 image exists at all
            from . import augment
            S = self._view_size = augment.view_size(sb["image_plan"])
            self._staged = (augment.stage_views(rt, sb["image_u8"], sb["image_hw"], sb["image_plan"], S, post=sb.get("image_post")), S, S)
            for k in ("image_u8", "image_hw", "image_plan") + (("image_post",) if "image_post" in sb else ()):
                sb[k] = torch.empty(sb[k].shape, dtype=sb[k].dtype, device="meta")
        else:
            from .resnet import stage_image
            img0 = sb["image"].to(torch.float32).contiguous()
            self._staged = (stage_image(rt, img0), img0.shape[2], img0.shape[3])
            sb["image"] = torch.empty(img0.shape, dtype=sb["image"].dtype, device="meta")      # shape / dtype witness for _fits only

        def image_fwd():
            keep["img"], keep["ctx_i"] = resnet_forward(rt, m.image_encoder.img_encoder, None, True, staged=self._staged)
            rt.bump_counters("image_encoder", 1)

        def text_fwd():
            # (first, on this stream: the tap-subset weights of the stride-2 dgrads — they depend on the weights only; in front of each class's
            # GEMM they were twelve small copies on the critical path of the image backward)
            from .resnet import s2_class_weights
            # the transposed weight copies of every input-gradient GEMM (Arena.register_transposed): one grouped launch per step, here — behind
            # the previous step's update in stream order, ahead of both backward passes (the image backward starts behind the heads' join)
            rt.arena.ensure_transposed(force=True, capturing=True)
            keep["ctx_i"]["s2w"] = keep["s2w"] = s2_class_weights(rt, m.image_encoder.img_encoder)
            keep["step_t"] = rt.next_step(True)
            keep["txt"], keep["ctx_t"] = bert_forward(rt, m.text_encoder.strans, sb["input_ids"], sb["attention_mask"], keep["step_t"])

        # the heads, cut along the modality boundary (loss.jsd_half_forward): the text half on the side stream right behind BERT, the image half
        # and the critic (the only joint piece) on the main stream
        from .loss import jsd_half_backward, jsd_half_block, jsd_half_forward, jsd_half_prior, jsd_join

        def heads_t1():
            keep["step_h"] = st = rt.next_step(True)
            # image prior noise, then text prior noise — the eager draw order (reference loss.py:189,196); a site is drawn only for an enabled
            # prior, exactly as loss.jsd_forward does, so that eager and replayed steps use the same sites whichever priors are on
            keep["sites"] = (st.site() if m.loss.image_prior else None, st.site() if m.loss.text_prior else None)
            keep["acc"] = torch.zeros(8, device=rt.device, dtype=torch.float32)
            keep["gout"] = torch.ones(1, device=rt.device, dtype=torch.float32)
            # the heads' weight gradients (9 Linear layers per modality incl. the priors: ~0.07 ms of latency-bound launches per chain) are collected:
            # the text half's ride in BERT's group, the image half's in a group of their own that replays with the first image segment's
            keep["wg_t"] = hip.WgradGroup(rt.dt, ws["t"], zeroed=True)
            keep["wg_h"] = hip.WgradGroup(rt.dt, ws["h"], zeroed=True)
            keep["dh_t"], keep["dh_i"] = (keep["wg_t"], keep["wg_h"]) if rt.defer_head_wgrads else (None, None)
            keep["ht"] = jsd_half_forward(rt, m.loss, keep["txt"], "text", st, keep["sites"][1], keep["acc"], keep["gout"], defer=keep["dh_t"])

        # the image half in two pieces that do not depend on each other: the prior discriminator (forward + backward, ~12 latency-bound launches)
        # on the side stream, idle between the text heads and the text backward, beside the MI block's forward on the main stream
        def heads_p1():
            keep["dprior_i"] = jsd_half_prior(rt, m.loss, keep["img"], "image", keep["step_h"], keep["sites"][0], keep["acc"], keep["gout"], defer=keep["dh_i"])

        def heads_b1():
            keep["hi"] = jsd_half_block(rt, m.loss, keep["img"], "image", keep["step_h"])

        def heads_m1():
            keep["hi"]["dprior"] = keep["dprior_i"]
            rt.bump_counters("loss", 2)
            out, keep["df1"], keep["df2"] = jsd_join(rt, m.loss, keep["hi"], keep["ht"], keep["acc"], keep["gout"])
            keep["out"] = out
            # views of the finalised accumulator, not copies: five copy nodes fewer between the critic and the image backward
            keep["result"] = {"loss": out[0], "loss_components": {"total_loss": out[0], "cross_modal_loss": out[1],
                                                                  "visual_loss": out[3], "textual_loss": out[4]}}

        def heads_m2():
            keep["dimg"] = jsd_half_backward(rt, keep["hi"], keep["df1"], defer=keep["dh_i"])

        def heads_t2():
            keep["dtxt"] = jsd_half_backward(rt, keep["ht"], keep["df2"], defer=keep["dh_t"])

        # image backward in chain segments with the weight gradients collected instead of launched (resnet_backward's `defer`): each segment's
        # replay as one grouped launch on the text encoder's stream — after BERT's backward, beside the HBM-bound BatchNorm chain of the
        # earlier stages on the main stream; only the last segment's (first block + stem) follow the chain on the main stream
        inet = m.image_encoder.img_encoder
        n1, n2 = len(inet.layer1), len(inet.layer2)
        # chain segments (first block index of each, walked backwards): [layer4, layer3] [layer2] [layer1, stem]. (Cutting layer1 per block so that
        # more of its weight gradients overlap the chain was measured slower, 18.9 vs 18.6 ms: a group of one block's four weight gradients
        # takes as long — 0.8 ms — as the group of all three blocks', which is the point of grouping.)
        cuts = [n1 + n2, n1, 0]
        segs = [f"s{i}" for i in range(len(cuts))]
        from . import hip
        ws = {k: hip.WgradGroup.alloc_workspace(rt.device) for k in segs + ["t", "h"]}      # pinned staging cannot be allocated inside a capture

        def image_bwd(i):
            def fn():
                # (zeroed: this capture visits every weight once per step and the update kernel leaves the gradient arena zeroed)
                keep["wg_" + segs[i]] = hip.WgradGroup(rt.dt, ws[segs[i]], zeroed=True)
                resnet_backward(rt, inet, keep["ctx_i"], keep["dimg"].contiguous() if i == 0 else None, defer=keep["wg_" + segs[i]],
                                stop_block=cuts[i], resume=i > 0)
            return fn

        def wgrad_heads():
            keep["wg_h"].launch()

        def wgrad(i):
            # the last segment's members that are launches of their own (layer1's three patch-resident 3 x 3 weight gradients, the stem's weight
            # gradient: ~0.35 ms) replay on the side stream, which is idle by then, beside the grouped launch on the main stream
            last = i == len(segs) - 1
            return lambda: keep["wg_" + segs[i]].launch(extras=not last)

        def wgrad_last_extras():
            keep["wg_" + segs[-1]].launch_extras()

        # BERT's backward: ONE graph with one weight-gradient group at its end when nothing is exchanged; under data parallel `text_segments` (3) chain
        # segments - pooler + layers 11..8 | 7..4 | 3..0 + embeddings - each with its own group, so that each segment's span of the gradient arena (the
        # text encoder is 438 of the step's 625 MB) goes to the exchange as soon as its graph is enqueued instead of behind the whole encoder (VERDICT r4
        # missing 2; reference train.py:174-178). One group per segment costs a little at one rank (grouping gains from size), hence only with an exchange.
        nts = int(getattr(self, "text_segments", 3 if self.exchange is not None else 1) or 1)
        nts = max(1, min(nts, len(m.text_encoder.strans.encoder.layer)))
        if m.text_encoder.strans.kind != "bert":
            nts = 1          # the MPNet tower's shared bias table is final only behind the first layer: its backward stays one segment
        tsegs = self._tsegs = [f"t{i}" for i in range(nts)]
        if nts > 1:
            ws.update({k: hip.WgradGroup.alloc_workspace(rt.device) for k in tsegs[1:]})

        def text_bwd(i):
            def fn():
                # (the text heads' weight gradients, collected in heads_t1 / heads_t2, ride in the first segment's group)
                g_ = keep["wg_t"] if i == 0 else hip.WgradGroup(rt.dt, ws[tsegs[i]], zeroed=True)
                keep["wg_" + tsegs[i]] = g_
                bert_backward(rt, m.text_encoder.strans, keep["ctx_t"], keep["dtxt"].contiguous() if i == 0 else None, defer=g_,
                              seg=(i, nts) if nts > 1 else None)
                g_.launch()
            return fn

        A0 = rt.arena
        img_span = A0.region("image_encoder.")

        def norm_early():
            # the gradient norm's early spans (text encoder, layer3 .. loss heads: final once the side stream's first weight-gradient group is done) on
            # the main stream behind its own last group - beside the side stream's last groups instead of behind them (0.1 ms of the 0.12 ms pass)
            if self.clip and self.clip > 0:
                self.inner._build_items()
                self.inner.zero_frozen()          # frozen tensors' unconditional gradients must not enter the norm
                self.inner.sumsq.zero_()
                hip_sumsq(self.inner, "early")

        def norm():
            self.inner.arena.join()
            if self.clip and self.clip > 0:
                self.inner.zero_frozen()          # (again: the late span's frozen tensors may have been written since)
                hip_sumsq(self.inner, "late")

        def update_img():                 # what the next image forward needs ...
            self.inner.launch(span=img_span)
            rt.end_capture()

        def update_rest():                # ... and the rest (text encoder, heads): arena order is text_encoder | image_encoder | loss
            self.inner.launch(span=(0, img_span[0]))
            self.inner.launch(span=(img_span[1], A0.total))

        rt.begin_capture()
        try:
            with torch.no_grad():
                capture("image_fwd", pool_main, image_fwd)
                capture("text_fwd", pool_side, text_fwd)
                capture("heads_t1", pool_side, heads_t1)
                capture("heads_p1", pool_side, heads_p1)
                capture("heads_b1", pool_main, heads_b1)
                capture("heads_m1", pool_main, heads_m1)
                capture("heads_t2", pool_side, heads_t2)
                capture("heads_m2", pool_main, heads_m2)
                for i, tg in enumerate(tsegs):
                    capture("text_bwd" if nts == 1 else "text_bwd_" + tg, pool_side, text_bwd(i))
                # Which stream replays a segment's grouped weight gradients: the side stream (behind BERT's backward) for every segment but the last, whose group
                # follows the chain on the main stream. (Round 5 built a switch that moved earlier segments' groups behind the whole chain: layer2's group there
                # cost 15.03 against 14.86 ms, and 14.94 against 14.59 in alternating order — whatever runs beside the chain slows it by less than the move
                # costs; the switch is gone. A third stream for the early groups: 14.88 against 14.72. The last segment's stand-alone launches on the main
                # stream instead of the side stream: no difference. DESIGN.md sections 0 and 8.)
                last = len(segs) - 1
                for i, sg in enumerate(segs):
                    capture("image_bwd_" + sg, pool_main, image_bwd(i))
                    if i == 0 and (keep["wg_h"].items or keep["wg_h"].extra):          # (never an empty capture: the A/B switch defer_head_wgrads=0 leaves the group empty)
                        capture("wgrad_heads", pool_side, wgrad_heads)          # (capture order = replay order on a stream: shared pool)
                    if i != last:
                        capture("wgrad_" + sg, pool_side, wgrad(i))
                capture("wgrad_" + segs[last], pool_main, wgrad(last))          # behind the chain
                # the last segment's stand-alone launches (bn1's backward + conv1's weight gradient, 0.2 ms): beside the last group, on the side stream
                if keep["wg_" + segs[-1]].extra:
                    capture("wgrad_last_extras", pool_side, wgrad_last_extras)
                if self.clip and self.clip > 0:          # (without clipping there is no norm: an empty capture is not worth finding out about)
                    capture("norm_early", pool_main, norm_early)
                capture("norm", pool_main, norm)
                capture("update_rest", pool_side, update_rest)
                capture("update_img", pool_main, update_img)
        except BaseException:
            rt.abort_capture()
            raise
        finally:
            rt.exchange = saved_exchange      # eager steps (a batch of another shape, eval) keep the overlapped exchange
        A = rt.arena
        self._regions = {k: A.region(k + ".") for k in ("text_encoder", "image_encoder", "loss")}
        # data parallel: the image encoder's gradients are exchanged per chain segment — stages 4 + 3 hold 22 M of its 23.5 M parameters and
        # are final 4 ms before the step ends (after the first weight-gradient group), so only stage 1 + stem (0.2 M) is exchanged exposed
        pre = "image_encoder.img_encoder."
        l2, l3, l4, img = A.region(pre + "layer2."), A.region(pre + "layer3."), A.region(pre + "layer4."), self._regions["image_encoder"]
        assert img[0] <= l2[0] <= l2[1] <= l3[0] <= l3[1] <= l4[0] <= l4[1] <= img[1]
        self._seg_spans = [(l3[0], img[1]), (l2[0], l3[0]), (img[0], l2[0])]          # s0 = [layer4, layer3], s1 = layer2, s2 = layer1 + stem
        if nts > 1:
            # arena order inside the text encoder: embeddings | layer 0 .. n - 1 | pooler; segment i covers layers [lo, hi) (+ the pooler for i = 0, + the
            # embeddings for the last one): contiguous spans, from the top
            from .bert import segment_layers
            tr, tp = self._regions["text_encoder"], "text_encoder.strans."
            nl = len(m.text_encoder.strans.encoder.layer)
            lay = [A.region(tp + f"encoder.layer.{j}.") for j in range(nl)]
            self._text_spans = []
            for i in range(nts):
                lo, hi = segment_layers(nl, (i, nts))
                self._text_spans.append((tr[0] if i == nts - 1 else lay[lo][0], tr[1] if i == 0 else lay[hi][0]))
            assert self._text_spans[0][1] == tr[1] and self._text_spans[-1][0] == tr[0] and all(a[0] == b[1] for a, b in zip(self._text_spans, self._text_spans[1:]))
        self.handover = []          # [(span, event recorded when its gradients were final)] of the last replay: tools/timeline_handover.py
        self._g, self._graphs, self._keep, self._static_out = graphs["update_img"], graphs, keep, keep["result"]
        self._segs = segs

    def _hand(self, span, stream):
        """Hand flat_g[span] to the exchange behind what is enqueued on `stream`; with track_handover also a timed event there (tools/timeline_handover.py)."""
        self.exchange.reduce_span(*span, after=stream)
        if getattr(self, "track_handover", False):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(stream)
            self.handover.append((span, ev))

    def _replay_direct(self):
        rt, G, ex = self.model.runtime, self._graphs, self.exchange
        main, side = torch.cuda.current_stream(rt.device), rt.side_stream
        if getattr(self, "track_handover", False):
            self.handover = []
            self._t0 = torch.cuda.Event(enable_timing=True)
            self._t0.record(main)
        side.wait_stream(main)
        G["image_fwd"].replay()
        with torch.cuda.stream(side):
            G["text_fwd"].replay()
            G["heads_t1"].replay()                 # text half of the heads: hidden under the tail of the image forward
            side.wait_stream(main)                 # (the image features)
            G["heads_p1"].replay()                 # image prior discriminator, forward + backward ...
        if self._rest_ev is not None:
            # the deferred update_rest (side stream, start of this step) rewrites the loss module's parameters, which heads_b1 reads on THIS stream:
            # only timing ordered the two (0.7 ms of update against 5 ms of image forward). The event has long fired by now: no cost
            main.wait_event(self._rest_ev)
            self._rest_ev = None
        G["heads_b1"].replay()                     # ... beside the image MI block's forward
        main.wait_stream(side)
        G["heads_m1"].replay()                     # critic forward + backward
        side.wait_stream(main)
        with torch.cuda.stream(side):
            G["heads_t2"].replay()                 # text block backward ...
            if len(self._tsegs) == 1:
                G["text_bwd"].replay()             # ... straight into BERT's backward
                if ex is not None:
                    self._hand(self._regions["text_encoder"], side)          # ordered after BERT's backward only (the event is taken now)
            else:
                for tg, span in zip(self._tsegs, self._text_spans):          # segment by segment: each span leaves while the next segment runs
                    G["text_bwd_" + tg].replay()
                    if ex is not None:
                        self._hand(span, side)
        G["heads_m2"].replay()                     # image block backward, beside it
        ev_early = None
        for i, sg in enumerate(self._segs[:-1]):   # a segment's weight gradients go to the side stream as soon as its chain is enqueued
            G["image_bwd_" + sg].replay()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                if i == 0:
                    # the image heads' weight gradients (collected by heads_p1 / heads_m2; the text heads' rode in BERT's group): behind BERT's
                    # backward and behind the main stream's heads_m2. Every gradient of the loss module is final after this launch
                    if "wgrad_heads" in G:
                        G["wgrad_heads"].replay()
                    if ex is not None:
                        self._hand(self._regions["loss"], side)
                G["wgrad_" + sg].replay()
                if i == 0:
                    ev_early = side.record_event()          # text encoder, loss heads, layer3 / layer4: the side stream's share of the norm's early spans
            if ex is not None:   # BatchNorm gradients came with the chain (main), weight gradients with the group (side, which waited for main)
                self._hand(self._seg_spans[i], side)
        G["image_bwd_" + self._segs[-1]].replay()
        side.wait_stream(main)
        if "wgrad_last_extras" in G:
            with torch.cuda.stream(side):
                G["wgrad_last_extras"].replay()    # bn1's backward + the stem's weight gradient, beside ...
        G["wgrad_" + self._segs[-1]].replay()      # ... the last grouped launch behind the chain
        early_done = ex is None and getattr(self, "norm_overlap", True) and "norm_early" in G
        if early_done:
            main.wait_event(ev_early)
            G["norm_early"].replay()               # beside the side stream's last groups
        if ex is not None:
            main.wait_stream(side)
            self._hand(self._seg_spans[-1], main)
            covered = sorted(self._regions.values())
            pos = 0
            for lo, hi in covered:                 # anything outside the three top-level modules (nothing, for VLInfoModel)
                if lo > pos:
                    ex.reduce_span(pos, lo, after=main)
                pos = max(pos, hi)
            if pos < rt.arena.total:
                ex.reduce_span(pos, rt.arena.total, after=main)
            ex.wait()
        main.wait_stream(side)
        if not early_done and "norm_early" in G:
            G["norm_early"].replay()               # (data parallel: only the exchanged gradients enter the norm; or norm_overlap = 0, the A/B)
        G["norm"].replay()
        G["update_img"].replay()
        if self.defer_update:
            self._pending_rest = True          # first thing of the next step, on the side stream (_replay), or finish()
        else:
            G["update_rest"].replay()

    def _capture_single(self, batch):
        rt = self.model.runtime
        self._static_batch = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in self._padded(batch).items()}
        self._view_size = None
        for k in ("image_plan", "neg_image_plan"):          # the view size is read here: inside the capture nothing may wait for the device
            if k in batch:
                from . import augment
                self._view_size = augment.view_size(batch[k])
        self.optimizer.zero_grad()            # no-op after a completed step (the update kernel leaves the gradients zeroed)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        saved_exchange, rt.exchange = rt.exchange, None      # no collectives inside a capture: the executors must not start buckets
        rt.begin_capture()
        try:
            with torch.cuda.graph(g, capture_error_mode="thread_local"):      # see _capture: other threads (pin-memory, RCCL) must not invalidate it
                # the transposed bf16 weight copies every input-gradient GEMM reads: re-derived INSIDE the graph, first on the capture stream (every
                # branch the executors fork is ordered behind it) — the backward executors' own ensure_transposed() is a no-op under capture, and
                # without this node every replay would run its dgrads against the weights of the last eager step
                rt.arena.ensure_transposed(force=True, capturing=True)
                sbatch = self._static_batch
                if self._view_size is not None:
                    sbatch = self.model.materialize_views(sbatch, size=self._view_size)
                out = self.model(sbatch)
                self.scaler.scale(out["loss"]).backward()
                if self.exchange is None:
                    self._capture_update()
                else:
                    self.inner.arena.join()
                rt.end_capture()
            if self.exchange is not None:
                g2 = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g2, pool=g.pool(), capture_error_mode="thread_local"):
                    self._capture_update()
                self._g_update = g2
        except BaseException:
            rt.abort_capture()
            raise
        finally:
            rt.exchange = saved_exchange
        self._g, self._static_out = g, out

    _CAPTION_KEYS = ("input_ids", "attention_mask", "neg_input_ids", "neg_attention_mask", "aug_input_ids", "aug_attention_mask")

    def _caption_fill(self, key):
        """What a caption tensor is padded with: the text tower's pad id for the ids (0 for BERT, 1 for MPNet), 0 for the masks."""
        st = getattr(getattr(self.model, "text_encoder", None), "strans", None)
        return int(getattr(st, "padding_idx", 0)) if key.endswith("input_ids") else 0

    def _padded(self, batch):
        """Caption tensors right-padded (ids with the pad id, masks with zeros: _caption_fill) to `pad_to` columns (see __init__); other entries untouched."""
        if not self.pad_to:
            return batch
        out = dict(batch)
        for k in self._CAPTION_KEYS:
            v = batch.get(k)
            if torch.is_tensor(v) and v.dim() == 2 and v.shape[1] < self.pad_to:
                w = torch.full((v.shape[0], self.pad_to), self._caption_fill(k), dtype=v.dtype, device=v.device)
                w[:, :v.shape[1]] = v
                out[k] = w
        return out

    def _fits(self, batch):
        """The batch can be fed to the captured step: same tensors, same shapes — caption tensors may be SHORTER than captured."""
        sb = self._static_batch
        for k, v in batch.items():
            if not torch.is_tensor(v):
                continue
            if k not in sb or not torch.is_tensor(sb[k]) or sb[k].dtype != v.dtype:
                return False
            if sb[k].shape == v.shape:
                continue
            if not (k in self._CAPTION_KEYS and v.dim() == 2 and v.shape[0] == sb[k].shape[0] and v.shape[1] < sb[k].shape[1]):
                return False
        return all(k in batch for k, v in sb.items() if torch.is_tensor(v))

    def _replay(self, batch):
        rt = self.model.runtime
        self.replays += 1
        sync = self.optimizer.advance() if hasattr(self.optimizer, "advance") else False
        alpha = getattr(self.optimizer, "alpha", 1.0)
        if self.exchange is not None:
            self.inner.grad_prescale = 1.0 / self.exchange.world
        # per-phase graphs: what only the side stream's graphs (captions) or the last graph (hyper-parameters) read is fed on the side stream,
        # off the main stream's critical path; the image is staged on the main stream, in front of its forward
        feed = rt.side_stream if self._graphs is not None else None
        if feed is not None:
            feed.wait_stream(torch.cuda.current_stream(rt.device))      # the previous step's update (main) read hp; its text graphs (side) the captions
            if self._pending_rest:            # the deferred share of the previous step's update: ahead of this step's hyper-parameter upload
                with torch.cuda.stream(feed):
                    self._graphs["update_rest"].replay()
                    self._rest_ev = feed.record_event()
                self._pending_rest = False
        for k, v in batch.items():
            if torch.is_tensor(v):
                dst = self._static_batch[k]
                if dst.device.type == "meta":           # the image: staged by one kernel into the buffer the captured stem reads
                    if k == "image":
                        from .resnet import stage_image
                        stage_image(rt, v.to(torch.float32).contiguous(), out=self._staged[0])
                    elif k == "image_u8":               # (its tables come with it)
                        from . import augment
                        augment.stage_views(rt, v, batch["image_hw"], batch["image_plan"], self._view_size, out=self._staged[0],
                                            post=batch.get("image_post"))
                    continue
                on_side = feed is not None and k in self._CAPTION_KEYS
                if on_side and v.is_cuda:
                    v.record_stream(feed)
                with torch.cuda.stream(feed) if on_side else contextlib.nullcontext():
                    if dst.shape == v.shape:
                        dst.copy_(v, non_blocking=True)
                    else:                               # a batch whose longest caption is shorter than the captured length
                        dst.fill_(self._caption_fill(k))
                        dst[:, :v.shape[1]].copy_(v, non_blocking=True)
        with torch.cuda.stream(feed) if feed is not None else contextlib.nullcontext():
            self.inner.upload_hp(sync, alpha, max_norm=self.clip if self.clip and self.clip > 0 else 0.0)
        rt.sync_graph_seeds()
        if self._graphs is not None:
            self._replay_direct()
        else:
            self._g.replay()
            if self.exchange is not None:
                self.exchange.reduce_all()
                self._g_update.replay()
        rt.arena._tr_stale = True          # the replayed update changed the weights: an eager step that follows re-derives the transposed copies
        self.scaler.update()
        self.scheduler.step()
        return self._static_out

    def __call__(self, batch):
        if not self.graph:
            return self._eager(batch)
        if self._g is None:
            if self._eager_steps < self.graph_warmup:
                self._eager_steps += 1
                return self._eager(batch)
            try:
                self._capture(batch)
            except Exception as e:      # noqa: BLE001
                self.graph, self._g, self._graphs = False, None, None
                torch.cuda.synchronize()
                if not self.allow_eager_fallback:
                    raise RuntimeError(f"hipGraph capture of the train step failed ({type(e).__name__}: {e}). Pass --no-hip-graph (TrainStep(graph=False)) "
                                       "to launch eagerly, or --allow-eager-fallback to continue after a failed capture.") from e
                logger.error(f"capture of the train step failed ({type(e).__name__}: {e}); continuing with eager launches (host-bound: ~20 ms of Python launches per step)")
                return self._eager(batch)
        if not self._fits(batch) or not self.model.training:
            return self._eager(batch)             # a batch of another shape (e.g. a ragged last one): same kernels, launched from Python
        return self._replay(batch)


def hip_sumsq(opt, part=None):
    opt.sumsq_spans(part)          # (FusedSGD.norm_spans: the same spans in the same order on every path)


def main(_A: argparse.Namespace):
    if _A.num_gpus_per_machine == 0 or not torch.cuda.is_available():
        raise RuntimeError("clip_lite_amd trains on MI355X GPUs only: the device math is HIP kernels and there is no CPU path "
                           "(the reference's own --num-gpus-per-machine 0 mode also fails: loss.py:186 calls .cuda())")
    device: Any = torch.device("cuda", torch.cuda.current_device())
    _C = Config(_A.config, _A.config_override)
    common_setup(_C, _A)
    if dist.is_master_process():
        make_directory(_A.checkpoints_dir + _C.RUN_ID)

    model = PretrainingModelFactory.from_config(_C).to(device)
    dist.broadcast_parameters(model)
    optimizer = OptimizerFactory.from_config(_C, model.named_parameters())
    scheduler = LRSchedulerFactory.from_config(_C, optimizer)
    scaler = GradScaler(enabled=_C.AMP)

    if _A.resume_from is not None:
        start_iteration = CheckpointManager(model=model, optimizer=optimizer, scheduler=scheduler, scaler=scaler).load(_A.resume_from)
    else:
        start_iteration = 0

    # reference train.py:150-172: a run resumed at or after the switch starts on the clustered loaders
    clusters = "clusters" in _C.DATA.NEGATIVE_SAMPLING
    if clusters:
        check_cluster_assets(_C)
    loader_type = "clusters" if clusters and start_iteration >= _C.DATA.NEGATIVE_SAMPLING_START_ITERATION else "normal"
    if loader_type == "clusters":
        logger.info("Starting clustered negative sampling, loading new dataloaders...")
    train_dataloader, val_dataloader = init_dataloaders(_C, _A, type=loader_type)
    train_dataloader_iter = cycle(train_dataloader, device, start_iteration, type=loader_type)

    exchange = None
    if dist.get_world_size() > 1:
        dist.synchronize()
        exchange = dist.GradientExchange(model.runtime.arena, algorithm=getattr(_A, "grad_exchange", "allreduce"))
        model.runtime.exchange = exchange

    timer = Timer(start_from=start_iteration + 1, total_iterations=_C.OPTIM.NUM_ITERATIONS)
    if dist.is_master_process():
        checkpoint_manager = CheckpointManager(_A.checkpoints_dir + _C.RUN_ID, model=model, optimizer=optimizer, scheduler=scheduler, scaler=scaler)

    # the caption length the step is captured at: the attention kernels' cap, 128 tokens for the BERT tower and 32 for MPNet (bert.bert_forward);
    # the CLIP text tower's own context length (cliptext.py)
    strans = getattr(getattr(model, "text_encoder", None), "strans", None)
    text_kind = getattr(strans, "kind", "bert")
    cap = strans.context_length if text_kind == "clip" else 128 if text_kind == "bert" else 32
    step = TrainStep(model, optimizer, scheduler, scaler, _C.OPTIM.CLIP_GRAD_NORM, exchange, graph=not _A.no_hip_graph,
                     pad_to=min(int(_C.DATA.MAX_CAPTION_LENGTH), cap), allow_eager_fallback=_A.allow_eager_fallback, defer_update=True)
    for iteration in range(start_iteration + 1, _C.OPTIM.NUM_ITERATIONS + 1):
        if clusters and iteration == _C.DATA.NEGATIVE_SAMPLING_START_ITERATION and loader_type == "normal":      # reference train.py:190-203
            logger.info("Starting clustered negative sampling, loading new dataloaders...")
            loader_type = "clusters"
            train_dataloader, val_dataloader = init_dataloaders(_C, _A, type="clusters")
            train_dataloader_iter = cycle(train_dataloader, device, iteration, type="clusters")
            step.recapture()           # the clustered batches do not fit the captured step: warm up and capture again on them
        timer.tic()
        batch = next(train_dataloader_iter)
        output_dict = step(batch)
        timer.toc()

        if iteration % _A.log_every == 0:
            loss = output_dict["loss"].item()          # host sync: off the timed path except on logging iterations
            logger.info(f"{timer.stats} [Loss {loss:.3f}] [GPU {dist.gpu_mem_usage()} MB]")
            if dist.is_master_process():
                comps = {k: float(v) for k, v in output_dict["loss_components"].items()}
                logger.info("train " + " ".join(f"{k}={v:.5f}" for k, v in comps.items()))

        if iteration % _A.checkpoint_every == 0:
            step.finish()          # the deferred share of the last update: before anything reads the parameters
            if dist.is_master_process():
                checkpoint_manager.step(iteration)
            dist.synchronize()
            torch.set_grad_enabled(False)
            model.eval()
            val_loss_counter: Counter = Counter()
            val_iteration = 0
            for val_iteration, val_batch in enumerate(val_dataloader, start=1):
                for key in val_batch:
                    val_batch[key] = val_batch[key].to(device)
                val_loss_counter.update(model(val_batch)["loss_components"])
            val_loss_dict = {k: v / max(val_iteration, 1) for k, v in dict(val_loss_counter).items()}
            dist.average_across_processes(val_loss_dict)
            torch.set_grad_enabled(True)
            model.train()
            if dist.is_master_process():
                logger.info("val " + " ".join(f"{k}={float(v):.5f}" for k, v in val_loss_dict.items()))

        if (iteration / _C.OPTIM.NUM_ITERATIONS) > 0.8 and iteration % _A.climax_freq == 0:
            step.finish()
            if dist.is_master_process():
                checkpoint_manager.climax_step(iteration)
            dist.synchronize()
    step.finish()


def cli():
    _A = build_parser().parse_args()
    if _A.num_gpus_per_machine == 0:
        main(_A)
    else:
        dist.launch(main, num_machines=_A.num_machines, num_gpus_per_machine=_A.num_gpus_per_machine, machine_rank=_A.machine_rank,
                    dist_url=_A.dist_url, args=(_A,))
