"""Which phase class runs a part of the schedule (`materialist_amd.routes`, asked by `optimize.optimize_envmap_ARMN`).  The tables were written
down, row by row, from the `if` chains the runners of `optimize_envmap_ARMN` held before the routes became functions (`env_phase_runner`,
`brdf_part_runner`): the class each of them constructed for the configuration.  No GPU, no native library."""
import pytest

from materialist_amd import routes

WHY = "4096 pixels: the layer kernels take whole 128-row tiles of at least 8192 rows"          # some ArmMlpPhase.why_not(...) that is not None
WHY_N = "predicted normals / a part that moves the normal map"                               # (what why_not says under predicted normals)

# model_name, use_mesh_normal, part, masked, batch (0: one [H,W,3] target), on_cuda, background, why_not -> the class under integrator "sh"
BRDF = [
    # none, one image on the GPU: the fused phase
    ("none", True, "rm", False, 0, True, False, None, "FusedBrdfPhase"),
    ("none", True, "a", False, 0, True, False, None, "FusedBrdfPhase"),
    ("none", True, "arm", False, 0, True, False, None, "FusedBrdfPhase"),
    ("none", True, "rm", False, 0, True, True, None, "FusedBrdfPhase"),             # pixels without geometry: no route of their own under `none`
    ("none", True, "rm", False, 0, False, False, None, "FusedBrdfPhase"),           # a CPU tensor whose part leaves the normals alone
    # predicted normals: a part that moves the normal map runs NormalBrdfPhase, one that leaves it alone the fused phase
    ("none", False, "n", False, 0, True, False, None, "NormalBrdfPhase"),
    ("none", False, "armn", False, 0, True, False, None, "NormalBrdfPhase"),
    ("none", False, "rm", False, 0, True, False, None, "FusedBrdfPhase"),
    ("none", False, "n", False, 8, True, False, None, "NormalBrdfPhase"),            # (before the batch is looked at)
    ("none", False, "n", False, 0, False, False, None, "BrdfPhase"),                 # ... but not on a CPU tensor
    ("none", False, "armn", False, 0, False, False, None, "BrdfPhase"),
    # mesh normals: the 'n' is dropped from the part; 'n' alone leaves nothing and goes to the autograd composition
    ("none", True, "rmn", False, 0, True, False, None, "FusedBrdfPhase"),
    ("none", True, "armn", False, 8, True, False, None, "PipelinedBrdfPhase"),
    ("none", True, "n", False, 0, True, False, None, "BrdfPhase"),
    ("none", True, "n", True, 3, True, False, None, "BrdfPhase"),
    # --use_mask: one image, a batch (before the pipelined route is looked at), predicted normals
    ("none", True, "rm", True, 0, True, False, None, "MaskedBrdfPhase"),
    ("none", True, "rm", True, 3, True, False, None, "MaskedBatchPhase"),
    ("none", True, "arm", True, 8, True, False, None, "MaskedBatchPhase"),
    ("none", True, "rm", True, 0, False, False, None, "MaskedBrdfPhase"),
    ("none", False, "rm", True, 0, True, False, None, "BrdfPhase"),
    ("none", False, "n", True, 0, True, False, None, "BrdfPhase"),
    ("none", False, "rm", True, 3, True, False, None, "BrdfPhase"),
    # batches: two groups on streams of their own for an even batch of at least 8 on the GPU
    ("none", True, "rm", False, 2, True, False, None, "FusedBrdfPhase"),
    ("none", True, "rm", False, 7, True, False, None, "FusedBrdfPhase"),
    ("none", True, "rm", False, 8, True, False, None, "PipelinedBrdfPhase"),
    ("none", True, "rm", False, 9, True, False, None, "FusedBrdfPhase"),
    ("none", True, "a", False, 10, True, False, None, "PipelinedBrdfPhase"),
    ("none", True, "rm", False, 8, False, False, None, "FusedBrdfPhase"),
    # pos_mlp: the launch-by-launch phase where ArmMlpPhase.why_not says nothing, else the autograd composition; predicted normals, or
    # pixels without geometry on an image the launch-by-launch phase does not take: PosMlpNormalPhase
    ("pos_mlp", True, "arm", False, 0, True, False, None, "ArmMlpPhase"),
    ("pos_mlp", True, "rm", True, 0, True, False, None, "ArmMlpPhase"),
    ("pos_mlp", True, "arm", False, 0, True, False, WHY, "PosMlpBrdfPhase"),
    ("pos_mlp", True, "arm", False, 0, False, False, "the image is not on a GPU", "PosMlpBrdfPhase"),
    ("pos_mlp", False, "armn", False, 0, True, False, WHY_N, "PosMlpNormalPhase"),
    ("pos_mlp", False, "rm", False, 0, True, True, WHY_N, "PosMlpNormalPhase"),
    ("pos_mlp", True, "arm", False, 0, True, True, None, "ArmMlpPhase"),
    ("pos_mlp", True, "arm", False, 0, True, True, WHY, "PosMlpNormalPhase"),
]

# model_name, integrator, batch, on_cuda, env_size, max_epochs -> the class
ENV = [
    ("none", "sh", 0, True, (16, 32), 5000, "EnvTexelPhase"),
    ("none", "sh", 0, True, (16, 32), 1, "EnvTexelPhase"),
    ("none", "sh", 0, True, (32, 32), 5000, "EnvTexelPhase"),                        # 1024 texels: still the texel phase
    ("none", "sh", 0, True, (32, 64), 5000, "FusedEnvPhase"),
    ("none", "sh", 0, True, (16, 65), 5000, "FusedEnvPhase"),
    ("none", "sh", 3, True, (16, 32), 5000, "FusedEnvPhase"),
    ("none", "sh", 1, True, (16, 32), 5000, "FusedEnvPhase"),                        # a [1,H,W,3] target is a batch
    ("none", "sh", 0, False, (16, 32), 5000, "FusedEnvPhase"),
    ("pos_mlp", "sh", 0, True, (16, 32), 5000, "EnvMlpPhase"),
    ("pos_mlp", "sh", 0, True, (32, 64), 1, "EnvMlpPhase"),
    ("pos_mlp", "sh", 0, False, (16, 32), 5000, "EnvMlpPhase"),
    ("none", "path", 0, True, (16, 32), 5000, "EnvHeadPhase"),
    ("none", "path", 0, True, (32, 64), 1, "EnvHeadPhase"),
    ("pos_mlp", "path", 0, True, (16, 32), 5000, "EnvHeadPhase"),
]


@pytest.mark.parametrize("row", BRDF, ids=lambda r: "-".join(str(x)[:12] for x in r[:-1]))
def test_brdf_route(row):
    model_name, use_mesh_normal, part, masked, batch, on_cuda, background, why_not, expected = row
    route, reason = routes.brdf_route(model_name, "sh", use_mesh_normal, part, masked, batch, on_cuda, background, why_not)
    assert route == expected and route in routes.BRDF_ROUTES and isinstance(reason, str)
    if expected in ("PosMlpBrdfPhase", "PosMlpNormalPhase"):
        assert reason == why_not                               # what the run's log gives as the reason
    # --integrator path: every part on the operator face, whatever the configuration
    route, reason = routes.brdf_route(model_name, "path", use_mesh_normal, part, masked, batch, on_cuda, background, why_not)
    assert route == ("PosMlpNormalPhase" if model_name == "pos_mlp" else "BrdfPhase")
    assert reason == "the fused phases model the deterministic render only"


@pytest.mark.parametrize("row", ENV, ids=lambda r: "-".join(str(x) for x in r[:-1]))
def test_env_route(row):
    *args, expected = row
    route, reason = routes.env_route(*args)
    assert route == expected and route in routes.ENV_ROUTES and isinstance(reason, str)
    if args[1] == "path":
        assert reason == "the fused env phase models the deterministic render only"


@pytest.mark.parametrize("max_epochs, on_cuda, graph", [(1, True, False), (8, True, False), (9, True, True), (5000, True, True), (9, False, False),
                                                          (5000, False, False)])
def test_env_graph(max_epochs, on_cuda, graph):
    assert routes.env_graph(max_epochs, on_cuda) is graph
    assert ("hipGraph" in routes.env_route("none", "sh", 0, on_cuda, (16, 32), max_epochs)[1]) is graph


def test_effective_part():
    assert routes.effective_part("armn", True) == "arm" and routes.effective_part("n", True) == "" and routes.effective_part("armn", False) == "armn"


def test_every_route_is_a_phase_class_and_offers_what_the_drive_loops_are_told():
    """`optimize.py` does not probe the phases: it knows from the route that the two envhead phases replay several iterations as one graph
    (`step_many`; `FusedEnvPhase` must not grow one: bench.py drives hot loop A by that attribute), that `EnvTexelPhase` writes its parameters
    back, and that `ArmMlpPhase` alone reports the iterations that really ran."""
    from materialist_amd import armhead, envhead, loop

    where = {"ArmMlpPhase": armhead, "EnvMlpPhase": envhead, "EnvTexelPhase": envhead}
    for name in routes.BRDF_ROUTES + routes.ENV_ROUTES:
        assert isinstance(getattr(where.get(name, loop), name), type), name
    assert hasattr(envhead.EnvMlpPhase, "step_many") and hasattr(envhead.EnvTexelPhase, "step_many") and not hasattr(loop.FusedEnvPhase, "step_many")
    assert hasattr(envhead.EnvTexelPhase, "sync_params") and not hasattr(envhead.EnvMlpPhase, "sync_params")
    assert hasattr(armhead.ArmMlpPhase, "iterations_run") and hasattr(armhead.ArmMlpPhase, "lr_at") and not hasattr(loop.PosMlpBrdfPhase, "iterations_run")
    for name in ("FusedBrdfPhase", "PipelinedBrdfPhase", "MaskedBrdfPhase", "MaskedBatchPhase", "NormalBrdfPhase"):
        assert all(hasattr(getattr(loop, name), m) for m in ("run", "poll", "lr_at", "current_maps")), name
