"""`optimize_envmap_ARMN` (inverse_img_w_mi.py:106-599) on the HIP render: the alternating env / BRDF optimisation of one image (`--model_name none`:
or a batch of independent images), both model modes and both integrators.  `schedule.run_schedule` decides which phase / part runs when,
`routes.env_route` / `routes.brdf_route` which phase class of `loop.py`, `armhead.py`, `envhead.py` runs it.  `_Inversion` holds what the parts of a
run share, constructs the phase a route names, drives it with one of two loops (`drive_polled`: EarlyStopping in device memory, read every
`sync_every` iterations; `drive_stepped`: one host check per epoch) and folds its best snapshot into the run's SaveBest (`fold_best`).  Frames,
best_results/ and the stage digests are written from here when the caller asks for them (`frames`, `results_dir`, `digests`)."""
from __future__ import annotations

import time
from typing import Callable, Dict, Optional, Sequence

import torch

from . import loop as _loop
from . import loss as _loss
from . import render as _render
from . import routes as _routes
from .armhead import ArmMlpPhase
from .envhead import EnvMlpPhase, EnvTexelPhase
from .schedule import run_schedule

ROUGHNESS_SHIFT, METALLIC_SHIFT = 0.7, 0.05   # :183-184
MAPS = ("albedo", "roughness", "metallic")


class _Inversion:
    """What the phases of one run share, and the runners `run_schedule` calls back (`env_phase`, `brdf_part`, `on_*`)."""

    def __init__(self, scene: _render.Scene, mat: Dict[str, torch.Tensor], params, gt: torch.Tensor, mask: Optional[torch.Tensor], originals, light: dict,
                 model_name: str, spp: int, scale_delta: float, sync_every: int, env_size: tuple, say, stage_digest, frames, results_dir, shading_normal):
        # `mat`: the current maps (every BRDF part ends by taking them back from `saver`); `params`: render.traverse(scene); `originals`: the
        # regulariser anchors; `light`: what hot loop A optimises (`env_params`) and the envmap it produces (`env_head()`: [He,We,3], a batch
        # [B,He,We,3]) -- none: `env_raw`, the texels before the softplus; pos_mlp: `env_net(start_envmap)`, and `brdf_net(start_arm)` for the maps
        self.scene, self.mat, self.params, self.gt, self.mask, self.originals = scene, mat, params, gt, mask, originals
        self.model_name, self.spp, self.scale_delta, self.sync_every, self.env_size = model_name, spp, scale_delta, sync_every, env_size
        self.say, self.stage_digest, self.frames, self.results_dir, self.shading_normal = say, stage_digest, frames, results_dir, shading_normal
        self.env_params, self.env_head, self.env_raw = light["env_params"], light["env_head"], light.get("env_raw")
        self.env_net, self.start_envmap, self.brdf_net, self.start_arm = (light.get(k) for k in ("env_net", "start_envmap", "brdf_net", "start_arm"))
        self.saver, self.routes = _loop.DeviceSaveBest(), []    # SaveBest is global across phases (F11); (loop, 'env' | 'brdf', part, route) as they ran
        # the best envmap after the last env phase; the light of the current BRDF phase; the last env phase's MSE; SaveBest's copy of brdf_net
        self.final_envmap = self.envmap4render = self.last_mse = self.best_brdf_weights = None

    def shown_normal(self) -> torch.Tensor:
        return self.shading_normal if self.shading_normal is not None else self.scene.shading_normal()

    def save_results(self) -> None:
        if self.results_dir is not None and self.gt.ndim == 3:
            from .pipeline import save_results

            save_results(self.results_dir, self.saver.best, self.mat.get("normal", self.shown_normal()))

    def fold_best(self, best_loss: torch.Tensor, tensors: Callable[[], Dict[str, torch.Tensor]]) -> bool:
        """Fold a phase's best loss (one per image) and its best tensors into the run's SaveBest; True when any image improved (:247,421-422).
        `tensors` is called only then: some of them are renders.  The merge is per image: images of a batch whose best loss did not improve
        keep their earlier snapshot.  The host-stepped routes hand the run's best loss to a saver of their own as a 0-d tensor
        (`.reshape(())`), which raises for more than one image, so they only ever get here with one, and for one image merging per image
        and replacing the snapshot wholesale are the same thing."""
        new, kept = best_loss.to(self.gt.device).reshape(-1), self.saver.best
        prev = self.saver.best_loss if self.saver.best_loss is not None else torch.full_like(new, float("inf"))
        improved = new < prev
        if not bool(improved.any()):
            return False
        self.saver.best_loss = torch.minimum(new, prev)
        for key, value in tensors().items():
            old = kept.get(key)
            if old is None or old.shape != value.shape or self.gt.ndim != 4:
                kept[key] = value.clone()
            else:
                kept[key] = torch.where(improved.to(value.device).reshape((-1,) + (1,) * (value.ndim - 1)), value, old)
        return True

    def fold_env_best(self, best_loss: torch.Tensor, envmap: torch.Tensor, rendered_img: Callable[[], torch.Tensor]) -> None:
        """SaveBest.update of hot loop A (:247): the maps it rendered with, its best envmap and the render under it."""
        tensors = lambda: dict({k: self.mat[k].detach() for k in MAPS}, envmap=envmap, rendered_img=rendered_img())
        if not self.fold_best(best_loss, tensors) and "envmap" not in self.saver.best:
            self.saver.best["envmap"] = envmap.clone()

    def reload_brdf_net(self, ph, merged: bool) -> None:
        if merged:
            self.best_brdf_weights = {k: v.clone() for k, v in ph.best_weights.items()}
        if self.best_brdf_weights is not None:
            self.brdf_net.load_state_dict(self.best_brdf_weights)                   # :586-587: reloaded after every part

    # ------------------------------------------------------------------ the two drive loops
    def drive_polled(self, ph, n_epochs: int, enqueue: Callable[[int, int], None], kind: str, frame: Callable[[int], None]):
        """SaveBest / EarlyStopping in device memory: `enqueue(done, k)` up to `sync_every` iterations, poll; -> (the state polled last, why it ended)"""
        done, stop = 0, "num_epochs"
        while done < n_epochs:
            k = min(self.sync_every, n_epochs - done)
            enqueue(done, k)
            done += k
            info = ph.poll()
            if self.frames is not None and self.gt.ndim == 3 and self.frames.due(kind):
                frame(done - 1)
            if bool(info["stopped"].all()):
                stop = "early_stop"
                break
        return ph.poll(), stop

    def drive_stepped(self, n_epochs: int, epoch: Callable[[int], bool]):
        """A host check every epoch, as the reference's (:250,428,550): `epoch(it)` runs one, True to stop; -> (the last epoch, why it ended)"""
        stop, it = "num_epochs", 0
        for it in range(n_epochs):
            if epoch(it):
                stop = "early_stop"
                break
        return it, stop

    # ------------------------------------------------------------------ hot loop A (:236-254)
    def env_phase(self, loop_num: int, lr_of, patience: int, min_delta: float, max_epochs: int):
        batch = self.gt.shape[0] if self.gt.ndim == 4 else 0
        route, reason = _routes.env_route(self.model_name, self.scene.integrator, batch, self.gt.is_cuda, self.env_size, max_epochs)
        self.routes.append((loop_num, "env", "", route))
        if route == "EnvHeadPhase":
            self.say(f"loop {loop_num}: env phase runs the autograd composition on the operator face (EnvHeadPhase) under the path-traced render "
                     f"(--integrator path, max_depth {self.scene.path['max_depth']}): {reason}")
            return self.env_phase_stepped(loop_num, lr_of, patience, min_delta, max_epochs)
        kw = dict(spp=self.spp, patience=patience, min_delta=min_delta, best_mse=self.saver.best_loss, history_len=max_epochs,
                  use_graph=_routes.env_graph(max_epochs, self.gt.is_cuda))
        if route == "FusedEnvPhase":
            opt = _loop.capturable_adam(self.env_params, lr_of(0)) if kw["use_graph"] else torch.optim.Adam(self.env_params, lr=lr_of(0))   # fresh Adam per loop (:225-229)
            ph = _loop.FusedEnvPhase(self.scene, self.gt, self.env_head, opt, **kw)
            set_lr, head_now = (lambda lr: _loop.set_lr(opt, lr)), (lambda: self.env_head().detach())
        elif route == "EnvMlpPhase":
            ph = EnvMlpPhase(self.scene, self.gt, self.env_net, self.start_envmap, lr=lr_of(0), env_size=self.env_size, **kw)
        else:
            ph = EnvTexelPhase(self.scene, self.gt, self.env_raw, lr=lr_of(0), **kw)
        if route != "FusedEnvPhase":          # the envhead phases: learning rate in device memory, `step_many`
            set_lr, head_now = ph.set_lr, ph.head
        lr_now = lr_of(0)

        def enqueue(done: int, k: int) -> None:
            nonlocal lr_now
            while k > 0:
                if lr_of(done) != lr_now:
                    lr_now = lr_of(done)
                    set_lr(lr_now)
                run = 1
                while route != "FusedEnvPhase" and run < k and lr_of(done + run) == lr_now:   # the iterations up to the next change of the learning rate
                    run += 1
                ph.step_many(run) if run > 1 else ph.step()                  # one graph of `run` unrolled iterations
                done, k = done + run, k - run

        info, stop = self.drive_polled(ph, max_epochs, enqueue, "env", lambda at: self.frames.env_frame(loop_num, at, self.gt, ph.pred, head_now()))
        if route == "EnvTexelPhase":
            ph.sync_params()                                                         # env_raw as an optimiser over it would have left it
        iters = int(info["iters"].max())
        self.fold_env_best(info["best_mse"], ph.best_env, lambda: ph.best_img)
        self.last_mse = float(ph.history()[iters - 1].max()) if iters > 0 else float("nan")
        return iters - 1, stop, self.last_mse

    def env_phase_stepped(self, loop_num: int, lr_of, patience: int, min_delta: float, max_epochs: int):
        opt = torch.optim.Adam(self.env_params, lr=lr_of(0))
        ph = _loop.EnvHeadPhase(self.scene, self.gt, self.env_head, opt, spp=self.spp, saver=_loop.DeviceSaveBest())
        if self.saver.best_loss is not None:
            ph.saver.best_loss = self.saver.best_loss.clone().reshape(())
        es, mse = (_loop.EarlyStopping(patience, min_delta) if patience > 0 else None), float("nan")

        def epoch(it: int) -> bool:
            nonlocal mse
            _loop.set_lr(opt, lr_of(it))
            mse = float(ph.step())
            if self.frames is not None and (it + 1) % self.sync_every == 0 and self.frames.due("env"):
                self.frames.env_frame(loop_num, it, self.gt, ph.pred, self.env_head().detach())
            if es is not None:
                es(mse)
            return es is not None and es.early_stop

        it, stop = self.drive_stepped(max_epochs, epoch)
        self.fold_env_best(ph.saver.best_loss, ph.saver.best["envmap"], lambda: ph.saver.best["rendered_img"])
        self.last_mse = mse
        return it, stop, mse

    def on_env_phase_end(self, loop_num: int, save: bool) -> None:
        best = self.saver.best
        self.final_envmap = best["envmap"].detach().clone()                         # :296
        if self.frames is not None and self.gt.ndim == 3 and "rendered_img" in best:
            self.frames.env_frame(loop_num, 9999, self.gt, best["rendered_img"] if best["rendered_img"].shape == self.gt.shape else self.gt,
                                  self.final_envmap, final=True)                    # opt_env_img.png (:298)
        if save:
            self.save_results()                                                     # :302-303
        self.stage_digest(f"loop {loop_num} env", self.final_envmap)
        self.say(f"loop {loop_num}: env phase done, mse {self.last_mse:.5f}")

    # ------------------------------------------------------------------ hot loop B (:347-468,470-590)
    def on_brdf_phase_begin(self, loop_num: int, which: str) -> None:              # :317-342
        env = self.final_envmap
        if which == "gt_or_ones":
            env = self.mat["gt_envmap"] if "gt_envmap" in self.mat else torch.ones(self.env_size + (3,), device=self.gt.device)
        self.params["emitter.data"] = self.envmap4render = env.detach()

    def brdf_part(self, loop_num: int, part: str, patience: int, min_delta: float, n_epochs: int):
        scene, gt = self.scene, self.gt
        why_not = ArmMlpPhase.why_not(scene, gt, self.brdf_net, part, self.mask) if self.model_name == "pos_mlp" else None
        route, reason = _routes.brdf_route(self.model_name, scene.integrator, scene.use_mesh_normal, part, self.mask is not None,
                                           gt.shape[0] if gt.ndim == 4 else 0, gt.is_cuda, scene.bg_mask is not None, why_not)
        self.routes.append((loop_num, "brdf", part, route))
        if scene.integrator == "path":
            how = "PosMlpNormalPhase with the network under autograd" if route == "PosMlpNormalPhase" else "BrdfPhase"
            self.say(f"loop {loop_num}: part {part!r} runs the autograd composition on the operator face ({how}) under the path-traced render "
                     f"(--integrator path, max_depth {scene.path['max_depth']}): {reason}")
        runner = self.brdf_part_stepped if route in ("BrdfPhase", "PosMlpNormalPhase") else \
            self.brdf_part_mlp if route in ("ArmMlpPhase", "PosMlpBrdfPhase") else self.brdf_part_polled
        return runner(route, reason, loop_num, part, patience, min_delta, n_epochs)

    def brdf_part_polled(self, route: str, reason: str, loop_num: int, part: str, patience: int, min_delta: float, n_epochs: int):
        """`none`, launch by launch on the C ABI with SaveBest / EarlyStopping on the device (no autograd)."""
        scene, gt, mat, moves_n = self.scene, self.gt, self.mat, route == "NormalBrdfPhase"
        kw = dict(optimize_part=_routes.effective_part(part, scene.use_mesh_normal), spp=self.spp, scale_delta=self.scale_delta, patience=patience,
                  min_delta=min_delta, best_mse=self.saver.best_loss, history_len=n_epochs, originals=self.originals)
        # the five classes take the same arguments, plus the normal map the part moves / the mask(s) / the number of groups stepping side by side
        extra = (mat["normal"],) if moves_n else (self.mask,) if route in ("MaskedBatchPhase", "MaskedBrdfPhase") else ()
        ph = getattr(_loop, route)(scene, gt, mat["albedo"], mat["roughness"], mat["metallic"], *extra, **kw,
                                   **({"groups": 2} if route == "PipelinedBrdfPhase" else {}))

        def frame(at: int) -> None:
            shown = ph.pred                                    # lazy loop: the render of the current parameters (the next iteration's)
            self.frames.mat_frame(loop_num, part, at, gt, _loss.linear_to_srgb((shown * (gt.mean() / shown.mean())).clamp_min(1e-8)),   # its own exposure ratio (:388)
                                  ph.current_maps(), ph.current_maps()["normal"] if moves_n else self.shown_normal())

        def best() -> Dict[str, torch.Tensor]:
            env4 = self.envmap4render
            if gt.ndim == 4 and env4.ndim == 3:
                env4 = env4.unsqueeze(0).expand((gt.shape[0],) + tuple(env4.shape))
            # SaveBest keeps the normal map it rendered with (:421-422)
            normal = ph.best["normal"] if moves_n else mat["normal"].detach() if not scene.use_mesh_normal and "normal" in mat else None
            return dict({k: ph.best[k] for k in MAPS}, rendered_img=ph.best_img, envmap=env4.contiguous(), **({} if normal is None else {"normal": normal}))

        info, stop = self.drive_polled(ph, n_epochs, lambda done, k: ph.run(k), "mat", frame)
        iters = int(info["iters"].max())
        if self.fold_best(info["best_mse"], best) and moves_n:
            mat["normal"] = self.saver.best["normal"]
        self.say(f"loop {loop_num}: part {part!r}{f' ({reason})' if moves_n else ''} ran {iters} iterations ({stop}), best mse {float(info['best_mse'].min()):.5f}")
        return iters - 1, ph.lr_at(max(iters - 1, 0)), stop

    def brdf_part_stepped(self, route: str, reason: str, loop_num: int, part: str, patience: int, min_delta: float, n_epochs: int):
        """The autograd render with the torch-composed loss and the reference's per-epoch host EarlyStopping: BrdfPhase (:335-340,378-379,406-409),
        PosMlpNormalPhase (output_type 'armn': the net predicts the normal map as well, :165-172,493-506); every part of `--integrator path`."""
        scene, mat, path = self.scene, self.mat, self.scene.integrator == "path"
        kw = dict(optimize_part=part, spp=self.spp, scale_delta=self.scale_delta, saver=_loop.DeviceSaveBest(), mask=self.mask)
        if route == "BrdfPhase":
            if not path:
                self.say(f"loop {loop_num}: part {part!r} runs the autograd composition on the operator face ({reason}): several times slower than the fused phases")
            ph = _loop.BrdfPhase(scene, self.gt, mat["albedo"], mat["roughness"], mat["metallic"], None if scene.use_mesh_normal else mat["normal"],
                                 originals=self.originals, **kw)
        else:
            ph = _loop.PosMlpNormalPhase(scene, self.gt, self.brdf_net, self.start_arm,
                                         {k: mat[k] for k in MAPS + (() if scene.use_mesh_normal else ("normal",))}, **kw)
            if not path and ph.engine is not None:
                self.say(f"loop {loop_num}: part {part!r} (pos_mlp, armn) runs launch by launch on the C ABI (PosMlpNormalPhase with armhead.MlpEngine: "
                         "render, losses, the network's layer products and AdamW; no autograd)")
            elif not path:
                self.say(f"loop {loop_num}: part {part!r} (pos_mlp) runs PosMlpNormalPhase with the network under autograd (render, losses and layer "
                         f"products on the C ABI), not a launch-by-launch phase: {reason}")
        if self.saver.best_loss is not None:
            ph.saver.best_loss = self.saver.best_loss.clone().reshape(())
        es = _loop.EarlyStopping(patience, min_delta)
        it, stop = self.drive_stepped(n_epochs, lambda it: es(float(ph.step())) or es.early_stop)      # (`es(...)` returns None)
        best = ph.saver.best
        merged = "albedo" in best and self.fold_best(ph.saver.best_loss, lambda: dict(
            {k: best[k] for k in MAPS + ("rendered_img", "normal") if k in best}, envmap=self.envmap4render))
        if merged and "normal" in best:
            mat["normal"] = self.saver.best["normal"]
        if route == "PosMlpNormalPhase":
            self.reload_brdf_net(ph, merged)
        self.say(f"loop {loop_num}: part {part!r} ({'with normals' if route == 'BrdfPhase' else 'pos_mlp, armn'}) ran {it + 1} iterations ({stop})")
        return it, ph.opt.param_groups[0]["lr"], stop

    def brdf_part_mlp(self, route: str, reason: str, loop_num: int, part: str, patience: int, min_delta: float, n_epochs: int):
        """pos_mlp under the geometric normals: the launch-by-launch phase, or the autograd composition where it does not apply."""
        gt, mat = self.gt, self.mat
        if route == "PosMlpBrdfPhase":        # not silently: the composition is several times slower than the launch-by-launch phase
            self.say(f"loop {loop_num}: part {part!r} (pos_mlp) runs the autograd composition, not the launch-by-launch phase: {reason}")
        ph = _loop.pos_mlp_brdf_phase(self.scene, gt, self.brdf_net, self.start_arm, {k: mat[k] for k in MAPS}, optimize_part=part, spp=self.spp,
                                      scale_delta=self.scale_delta, patience=patience, min_delta=min_delta, best_mse=self.saver.best_loss,
                                      history_len=n_epochs, mask=self.mask)

        def epoch(it: int) -> bool:
            if ph.step_and_check():                                                 # per-epoch host check, as the reference (:550)
                return True
            if self.frames is not None and it % 10 == 0 and self.frames.due("mat"):
                self.frames.mat_frame(loop_num, part, it, gt, _loss.linear_to_srgb((ph.pred * ph.stats[0, 0]).clamp_min(1e-8)),
                                      {k: ph.best[k] for k in MAPS}, self.shown_normal())
            return False

        it, stop = self.drive_stepped(n_epochs, epoch)
        best = ph.stats[:, ph.ops.STAT_BEST].clone()
        self.reload_brdf_net(ph, self.fold_best(best, lambda: dict({k: ph.best[k] for k in MAPS}, rendered_img=ph.best_img,
                                                                   envmap=self.envmap4render)))
        if route == "ArmMlpPhase":
            # the device-side EarlyStopping is polled every few iterations: the iterations enqueued between the stop and the poll were no-ops,
            # so the epoch and the learning rate reported are those of the last iteration that really ran
            it = max(ph.iterations_run - 1, 0)
        lr_end = ph.lr_at(it) if route == "ArmMlpPhase" else ph.opt.param_groups[0]["lr"]
        self.say(f"loop {loop_num}: part {part!r} (pos_mlp) ran {it + 1} iterations ({stop}), best mse {float(best.min()):.5f}")
        return it, lr_end, stop

    def on_brdf_part_end(self, loop_num: int, part: str) -> None:                  # :460-463: every map comes back from the saver
        mat, params = self.mat, self.params
        for key in MAPS:
            mat[key] = self.saver.best[key].detach().clone()
        params["shape.bsdf.a"], params["shape.bsdf.r"], params["shape.bsdf.m"] = mat["albedo"], mat["roughness"], mat["metallic"]
        if not self.scene.use_mesh_normal and "normal" in self.saver.best:
            mat["normal"] = self.saver.best["normal"].detach().clone()
            params["shape.bsdf.n"] = mat["normal"]
        elif self.scene.integrator == "path" and not self.scene.use_mesh_normal and "normal" in mat:
            # no snapshot holds a normal map yet (no part has improved on the env phase's loss): the scene still has the part's last
            # iterate, a node of a graph that is gone, and the next env phase renders through PathRenderFn, which differentiates its normals
            params["shape.bsdf.n"] = mat["normal"] = mat["normal"].detach()
        self.save_results()                                                         # :465,590
        self.stage_digest(f"loop {loop_num} brdf {part}", mat["albedo"], mat["roughness"], mat["metallic"])


def optimize_envmap_ARMN(scene: _render.Scene, mat: Dict[str, torch.Tensor], optimize_order: Sequence[str] = ("arm",), spp: int = 64,
                         opt_env_from: int = 0, opt_src: str = "arm", scale_delta: float = 0.1, num_epochs: int = 5000,
                         sync_every: int = 25, env_size=(16, 32), log=None, frames=None, results_dir: Optional[str] = None,
                         shading_normal: Optional[torch.Tensor] = None, model_name: str = "none", use_mask: bool = False,
                         digests: Optional[list] = None) -> Dict[str, object]:
    """mat: albedo [H,W,3], roughness [H,W,1], metallic [H,W,1], normal [H,W,3], gt_image [H,W,3] (optionally gt_envmap).
    Returns the best maps / envmap / render, the final PSNR, the schedule trace and the route every phase / part took (`routes`).  `frames`
    (pipeline.FrameWriter) and `results_dir` switch on the reference's file outputs: a frame at every host poll (the reference: every 10
    epochs, :257,438,559) and best_results/ after each phase (:302-303,465,590)."""
    gt, mat = mat["gt_image"].contiguous(), dict(mat)
    dev = gt.device
    # `digests` (a list the caller hands in): (stage, SHA-256 of the stage's tensors) at the schedule's boundaries -- what a run that came out
    # different is compared on to find the FIRST stage that differs (tools/pipeline_hashes.py, tests/golden/indoor2_digests.json).  A stage
    # boundary already synchronises with the host (the pollers have returned), so the copies cost nothing the loops would notice
    stage_digest = (lambda stage, *tensors: digests.append((stage, _loss.tensors_digest(*tensors)))) if digests is not None else (lambda *_: None)
    stage_digest("inputs", gt, mat["albedo"], mat["roughness"], mat["metallic"], scene.shading_normal())
    if "r" not in opt_src:                                                         # :185-188
        mat["roughness"] = torch.full_like(mat["roughness"], ROUGHNESS_SHIFT)
    if "m" not in opt_src:
        mat["metallic"] = torch.full_like(mat["metallic"], METALLIC_SHIFT)
    params = _render.traverse(scene)                                               # :216-220
    params["shape.bsdf.a"], params["shape.bsdf.r"], params["shape.bsdf.m"] = mat["albedo"], mat["roughness"], mat["metallic"]
    if not scene.use_mesh_normal:                                                  # 'n' in opt_order: shade with the predicted normal map (:335-340)
        mat["normal"] = torch.nn.functional.normalize(mat["normal"], p=2, dim=-1)  # :193
        params["shape.bsdf.n"] = mat["normal"]
    # regulariser anchors albedo_ori / roughness_ori / metallic_ori / normal_ori: captured ONCE, before the loops (:189-201), and
    # used by every part of every loop (:398-409) -- not the previous part's best maps
    originals = {k: mat[k].detach().clone() for k in MAPS + (() if scene.use_mesh_normal else ("normal",))}
    mask = mat.get("mask") if use_mask else None                                   # --use_mask (:379-381,509-511,702-711)
    if use_mask and mask is None:
        raise ValueError("use_mask needs mat['mask'] ([H,W] bool)")
    env_size = tuple(env_size)
    if model_name == "pos_mlp":                                                     # :114-124,159-172,179-207
        from . import posmlp

        if gt.ndim != 3:
            raise NotImplementedError("pos_mlp mode optimises one image per call")
        env_net = posmlp.envmap_net().to(dev)
        start_envmap = torch.ones(env_size[0] * env_size[1], 3, device=dev)
        armn = not scene.use_mesh_normal                                            # output_type (:159-172,203-206)
        brdf_net = posmlp.brdf_net("armn" if armn else "arm").to(dev)
        start_arm = torch.cat([mat["albedo"].reshape(-1, 3), mat["roughness"].reshape(-1, 1), mat["metallic"].reshape(-1, 1)], dim=-1)
        start_arm = torch.cat([start_arm, mat["normal"].reshape(-1, 3)], dim=-1) if armn else start_arm.clamp(0, 1)
        light = dict(env_net=env_net, start_envmap=start_envmap, env_params=list(env_net.parameters()), brdf_net=brdf_net, start_arm=start_arm,
                     env_head=lambda: env_net(start_envmap).reshape(env_size + (3,)))
    elif model_name == "none":
        # one light per image: a batch of independent images ([B,H,W,3] target) optimises B envmaps side by side
        lead = (gt.shape[0],) if gt.ndim == 4 else ()
        env_raw = torch.zeros(lead + env_size + (3,), dtype=torch.float32, device=dev, requires_grad=True)
        light = dict(env_raw=env_raw, env_params=[env_raw], env_head=lambda: torch.nn.functional.softplus(env_raw))
    else:
        raise ValueError("model_name should be 'none' or 'pos_mlp'")
    t_start = time.perf_counter()
    say = (lambda msg: log(f"[{time.perf_counter() - t_start:7.2f} s] {msg}")) if log is not None else (lambda *_: None)
    run = _Inversion(scene, mat, params, gt, mask, originals, light, model_name, spp, scale_delta, sync_every, env_size, say, stage_digest, frames,
                     results_dir, shading_normal)
    trace = run_schedule(list(optimize_order), None, None, opt_src=opt_src, opt_env_from=opt_env_from, num_epochs=num_epochs,
                         on_env_phase_end=run.on_env_phase_end, on_brdf_phase_begin=run.on_brdf_phase_begin, on_brdf_part_end=run.on_brdf_part_end,
                         brdf_part_runner=run.brdf_part, env_phase_runner=run.env_phase)
    best, saver = run.saver.best, run.saver
    with torch.no_grad():
        params["emitter.data"] = best["envmap"]
        final = _render.render_w_brdf(scene, best["albedo"], best["roughness"], best["metallic"], None if scene.use_mesh_normal else mat["normal"], spp)
        red = (-3, -2, -1) if gt.ndim == 4 else None                                # per image for a batch
        ratio = gt.mean(dim=red, keepdim=True) / final.mean(dim=red, keepdim=True) if red else gt.mean() / final.mean()
        psnr_each = _loss.psnr(final * ratio, gt).reshape(-1)
    stage_digest("final", best["albedo"], best["roughness"], best["metallic"], best["envmap"], final)
    return {"albedo": best["albedo"], "roughness": best["roughness"], "metallic": best["metallic"], "normal": mat.get("normal"),
            "envmap": best["envmap"], "rendered_img": best["rendered_img"], "final_render": final,
            "psnr": float(psnr_each.mean()), "psnr_per_image": psnr_each.tolist(), "best_loss": float(saver.best_loss.min()),
            "best_loss_per_image": saver.best_loss.reshape(-1).tolist(), "trace": trace, "routes": run.routes}
