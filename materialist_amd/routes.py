"""Which phase class runs a part of the schedule, as pure functions of plain values (no tensors, no scene): `optimize.py` asks them once per env
phase / BRDF part (tests/test_routes.py holds the table).  `route`: the name of the class that is constructed; `reason`: the clause the run's
log gives for it, or a word on what set the route where the log says nothing."""
from typing import Optional, Sequence, Tuple

BRDF_ROUTES = ("FusedBrdfPhase", "PipelinedBrdfPhase", "MaskedBrdfPhase", "MaskedBatchPhase", "NormalBrdfPhase", "BrdfPhase", "ArmMlpPhase", "PosMlpBrdfPhase", "PosMlpNormalPhase")
ENV_ROUTES = ("EnvMlpPhase", "EnvTexelPhase", "FusedEnvPhase", "EnvHeadPhase")


def effective_part(part: str, use_mesh_normal: bool) -> str:
    """Under the geometric normals an 'n' in the part optimises nothing (inverse_img_w_mi.py:356,376)."""
    return part.replace("n", "") if use_mesh_normal else part


def brdf_route(model_name: str, integrator: str, use_mesh_normal: bool, part: str, masked: bool, batch: int, on_cuda: bool, background: bool,
               why_not: Optional[str]) -> Tuple[str, str]:
    """`batch`: 0 for a single [H,W,3] target, else the number of images; `background`: the scene has pixels without geometry;
    `why_not`: what `ArmMlpPhase.why_not(...)` returned (pos_mlp only)."""
    if integrator == "path":                  # the path-traced render: every part on the operator face (its autograd compositions)
        return ("PosMlpNormalPhase" if model_name == "pos_mlp" else "BrdfPhase"), "the fused phases model the deterministic render only"
    if model_name == "pos_mlp":
        # predicted normals, or pixels without geometry on an image the launch-by-launch phase does not take: the operator face
        if not use_mesh_normal or (background and why_not is not None):
            return "PosMlpNormalPhase", why_not or ""
        return ("ArmMlpPhase", "") if why_not is None else ("PosMlpBrdfPhase", why_not)    # (chosen again by loop.pos_mlp_brdf_phase)
    # Under a FIXED predicted normal map (use_mesh_normal False, no 'n' in the part) the fused phases shade with it as they do with the geometric
    # normals; a part that MOVES the normal map runs NormalBrdfPhase (launch by launch on the C ABI, device-side SaveBest / EarlyStopping); what is
    # left -- masks with predicted normals, a part that is 'n' alone under the geometric normals -- is the autograd composition's
    eff = effective_part(part, use_mesh_normal)
    if not eff or (masked and not use_mesh_normal) or ("n" in eff and not on_cuda):
        return "BrdfPhase", "a mask under predicted normals, or 'n' alone under the geometric normals"
    if "n" in eff:
        return "NormalBrdfPhase", "normal map, on the device"
    if masked:                                # a batch under --use_mask: its images alone, each on a stream of its own
        return ("MaskedBatchPhase", "a batch under --use_mask") if batch else ("MaskedBrdfPhase", "--use_mask")
    if batch >= 8 and batch % 2 == 0 and on_cuda:     # a shard of images: two groups stepping on streams of their own
        return "PipelinedBrdfPhase", "an even batch of at least 8"
    return "FusedBrdfPhase", ""


def env_graph(max_epochs: int, on_cuda: bool) -> bool:     # the device env phases capture their iteration into a hipGraph after three eager ones
    return max_epochs > 8 and on_cuda


def env_route(model_name: str, integrator: str, batch: int, on_cuda: bool, env_size: Sequence[int], max_epochs: int) -> Tuple[str, str]:
    if integrator == "path":
        return "EnvHeadPhase", "the fused env phase models the deterministic render only"
    how = "one hipGraph per replay" if env_graph(max_epochs, on_cuda) else "eager launches"
    if model_name == "pos_mlp":               # the reference's parameterisation (envmap_net, :117-124,238-239), every launch on the C ABI
        return "EnvMlpPhase", how
    if not batch and on_cuda and env_size[0] * env_size[1] <= 1024:    # the texels through a softplus: head, its backward and Adam on the C ABI too
        return "EnvTexelPhase", how
    return "FusedEnvPhase", how
