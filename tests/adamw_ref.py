"""AdamW oracles shared by the bit-level AdamW tests (helper of the tests, not a test)."""
import numpy as np
import torch

from oracle import unet_ref_cpu as O


class IeeeSqrtAdamW(O.AdamWState):
    """The oracle's AdamW (torch's CPU ops, op for op) with a correctly rounded sqrt: this
    host's vectorised torch.sqrt is 1 ulp low on ~0.7 % of fp32 inputs (measured against
    IEEE sqrt; a host-library property, not part of the algorithm)."""

    def step(self, params, grads):
        import math
        self.step_count += 1
        b1, b2 = self.betas
        bc1 = 1 - b1 ** self.step_count
        bc2 = 1 - b2 ** self.step_count
        step_size = self.lr / bc1
        bc2_sqrt = math.sqrt(bc2)
        with torch.no_grad():
            for k, p in params.items():
                g = grads[k]
                p.mul_(1 - self.lr * self.wd)
                self.m[k].lerp_(g, 1 - b1)
                self.v[k].mul_(b2).addcmul_(g, g, value=1 - b2)
                sq = torch.from_numpy(np.sqrt(self.v[k].numpy()))
                denom = (sq / bc2_sqrt).add_(self.eps)
                p.addcdiv_(self.m[k], denom, value=-step_size)


def scaled_grad(g, grad_scale):
    """g * float32(grad_scale), rounded once in fp32 -- adamw_elem's first line."""
    if grad_scale == 1.0:
        return g.clone()
    return torch.from_numpy(g.numpy() * np.float32(grad_scale))


def oracle_step(p, g, m, v, step, lr, betas, eps, wd, grad_scale=1.0):
    """One AdamW step number `step` from the host state (p, g, m, v), by both oracles.
    Returns (p_torch, p_ieee, m, v): the moments of the two oracles are the same tensors' worth
    of ops, so one pair is returned (the torch oracle's)."""
    gs = scaled_grad(g, grad_scale)
    out = []
    for cls in (O.AdamWState, IeeeSqrtAdamW):
        o = cls({"a": p}, lr=lr, betas=betas, eps=eps, weight_decay=wd)
        o.m["a"], o.v["a"] = m.clone(), v.clone()
        o.step_count = step - 1
        P = {"a": p.clone()}
        o.step(P, {"a": gs})
        out.append((P["a"], o.m["a"], o.v["a"]))
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])
    return out[0][0], out[1][0], out[0][1], out[0][2]


def assert_step_matches(got_p, got_m, got_v, p_in, p_ref, p_ieee, m_ref, v_ref, lr, wd, tag=""):
    """The assertions of test_gpu_parity.py::test_adamw_bitwise_vs_oracle for one step:
    exp_avg / exp_avg_sq bit-equal to the torch-CPU oracle, params bit-equal to the IEEE-sqrt
    oracle, and every difference from the pure-torch oracle explained (and bounded) by the
    host's sqrt.  Returns the number of params that differ from the torch-CPU oracle."""
    assert torch.equal(got_m, m_ref), f"{tag}: exp_avg differs on {(got_m != m_ref).sum().item()}"
    assert torch.equal(got_v, v_ref), f"{tag}: exp_avg_sq differs on {(got_v != v_ref).sum().item()}"
    assert torch.equal(got_p, p_ieee), \
        f"{tag}: {(got_p != p_ieee).sum().item()} params differ from the IEEE-sqrt oracle"
    diff = got_p != p_ref
    hs, ies = torch.sqrt(v_ref), torch.from_numpy(np.sqrt(v_ref.numpy()))
    host_sqrt_off = hs != ies
    assert bool(torch.all(host_sqrt_off[diff])), f"{tag}: a difference not explained by the host sqrt"
    k = int((hs.view(torch.int32).long() - ies.view(torch.int32).long()).abs().max())
    u = p_ieee.double() - p_in.double() * (1 - lr * wd)
    dp = (got_p.double() - p_ref.double()).abs()
    bound = 8 * k * 2.0 ** -23 * u.abs() + torch.from_numpy(np.spacing(p_ref.abs().numpy())).double()
    assert bool(torch.all(dp <= bound)), f"{tag}: {float((dp / bound).max()):.2f} x the bound"
    return int(diff.sum())
