"""Plain torch restatement of the envmap MLP's backward chain (`envhead.EnvMlpPhase`: one `matpbr_mlp_small_bwd_step` per layer behind
`matpbr_env_project_bwd`), written for fp64 and checked against torch autograd on the CPU (tests/test_env_fp64_host.py).  The GPU tests
(tests/test_gpu_env_grad.py) compare the kernels with these helpers launch by launch.  Nothing here needs a GPU or the native library;
every function follows the dtype of what it is given, so the same code is the fp32 composition the bounds are measured against."""
import torch
import torch.nn.functional as F


def bwd_step64(g, w, c_prev, x, colsum_rows=32):
    """One backward step of a sine layer, given g = dL/d pre of the layer [M, n_red]:
        d_w    = g^T x                      x [M, K] the layer's input
        g_prev = (g w) * c_prev             w [n_red, n_prev] the layer's FORWARD weight (its columns that read the layer below),
                                            c_prev [M, n_prev] the cosines of the layer below; None, None without w
        colsum = column sums of g_prev over each tile of `colsum_rows` rows, [ceil(M / colsum_rows), n_prev]
        d_bias = g.sum(0)
    Returns (d_w, g_prev, colsum, d_bias)."""
    d_w = g.t() @ x
    d_bias = g.sum(0)
    if w is None:
        return d_w, None, None, d_bias
    g_prev = (g @ w) * c_prev
    M = g.shape[0]
    colsum = torch.stack([g_prev[r:r + colsum_rows].sum(0) for r in range(0, M, colsum_rows)])
    return d_w, g_prev, colsum, d_bias


def softplus_grad64(y):
    """d softplus(y) / d y as torch.nn.functional.softplus (beta 1, threshold 20) defines it: the sigmoid up to 20, exactly 1 above."""
    return torch.where(y > 20, torch.ones_like(y), torch.sigmoid(y))


def project64(y, proj):
    """env = softplus(y[:, :3]) [T, 3], light = proj env [25, 3]; proj [25, T] the SH projection of the texel grid."""
    env = F.softplus(y[:, :3])
    return env, proj @ env


def project_bwd64(y, proj, d_light):
    """d_y [T, 3] = (proj^T d_light) * softplus'(y[:, :3])."""
    return (proj.t() @ d_light) * softplus_grad64(y[:, :3])


def layers_of(net):
    """[(name prefix, Linear)] of a PosMLP, first layer first (the last layer has no `.linear`)."""
    L = net.n_layers
    out = []
    for l in range(L):
        layer = getattr(net, f"lin{l}")
        out.append((f"lin{l}.linear", layer.linear) if l < L - 1 else (f"lin{l}", layer))
    return out


def forward64(weights, biases, skip, x0):
    """Pre-activation of the output layer y [M, n_out], the input of every layer and the cosine of every sine layer's pre-activation.
    A layer listed in `skip` reads cat(sines of the layer below, x0), as `envhead` lays its buffers out."""
    L = len(weights)
    inp, inps, coss = x0, [], []
    for l in range(L):
        inps.append(inp)
        pre = torch.addmm(biases[l], inp, weights[l].t())
        if l == L - 1:
            return pre, inps, coss
        coss.append(torch.cos(pre))
        inp = torch.sin(pre)
        if (l + 1) in skip:
            inp = torch.cat([inp, x0], dim=1)


def chain64(net, x0, d_y):
    """The whole backward pass of a PosMLP(output_type='envmap') behind its softplus, as repeated `bwd_step64`: d_y [M, n_out] = dL/d(output
    pre-activations) -> {parameter name: gradient}.  The skip concatenation as `envhead` handles it: the weight gradient of a skip layer is
    taken against the whole concatenated input, the gradient into the layer below through the weight's first n_prev columns only."""
    lins = layers_of(net)
    weights = [lin.weight.detach() for _, lin in lins]
    biases = [lin.bias.detach() for _, lin in lins]
    _, inps, coss = forward64(weights, biases, net.skip, x0)
    grads, g = {}, d_y
    for l in range(len(lins) - 1, -1, -1):
        if l > 0:
            n_prev = weights[l - 1].shape[0]
            d_w, g_prev, _, d_b = bwd_step64(g, weights[l][:, :n_prev], coss[l - 1], inps[l])
        else:
            d_w, g_prev, _, d_b = bwd_step64(g, None, None, inps[l])
        grads[lins[l][0] + ".weight"], grads[lins[l][0] + ".bias"] = d_w, d_b
        g = g_prev
    return grads
