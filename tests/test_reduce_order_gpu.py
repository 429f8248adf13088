"""GPU tier: the fixed summation ORDER of the training reductions' second stage (csrc/cmr_reduce.h), bit for bit.  The data-parallel ranks
stay identical only while every rank adds the same partials in the same order; the other tests compare against float64 within a tolerance
and would not see an order change.  Two public ops take the partials from outside and return pure sums, so numpy can restate their order
exactly (float64 addition is IEEE on both sides):
  * ops.wgrad_group's vector jobs -- the strided-slice sum (4 slice groups, 8 loads in flight) and its LDS combine;
  * ops.bn_bwd_from_sums' dgamma / dbeta -- the wave-of-partials sum and the xor butterfly.
The partials are of mixed magnitude (1e-3 .. 1e3, both signs); each restatement is first held against math.fsum of the same numbers to one
fp32 ulp: that it adds the right operands needs no GPU.  Sums of such fp32 values are EXACT in float64 (24 + 20 + 7 bits), so these cases
pin the operands, the tails, the fp32 rounding and the accumulate step but no order of float64 additions can show in them.  Every case
is therefore run a second time with a pair +B, -B (|B| ~ 2^40 .. 2^43) planted in two slices of every output: the running sum between
the two is rounded to B's float64 ulp (~1e-4), which leaves a different fp32 result for (nearly) every other order of the additions."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def mixed(rng, shape):
    """fp32 values with |v| log-uniform in [1e-3, 1e3) and a random sign"""
    return (10.0 ** rng.uniform(-3.0, 3.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def plant_pairs(rng, part):
    """part [nparts >= 2, n] with +B and -B written over two distinct random slices of every column"""
    part = part.copy()
    for i in range(part.shape[1]):
        j1, j2 = rng.choice(part.shape[0], size=2, replace=False)
        b = np.float32(rng.uniform(1.0, 8.0) * 2.0 ** 40)
        part[j1, i], part[j2, i] = b, -b
    return part


def check_rounded_sum(restated, operands):
    """restated [n] float64 against math.fsum: within the bound of a recursive float64 sum in any order, (parts - 1) 2^-53 sum |x|"""
    for i in range(restated.shape[0]):
        col = [float(v) for v in operands[:, i]]
        assert abs(restated[i] - math.fsum(col)) <= (len(col) - 1) * 2.0 ** -53 * math.fsum(abs(v) for v in col), i


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def check_is_the_sum(restated, operands):
    """restated [n] float64 against math.fsum over operands [parts, n], both rounded to fp32: within one fp32 ulp"""
    for i in range(restated.shape[0]):
        exact = np.float32(math.fsum(float(v) for v in operands[:, i]))
        assert abs(np.float32(restated[i]) - exact) <= np.spacing(np.abs(exact)), (i, restated[i], exact)


def slice_group_sum(part, grp):
    """per column of part [nparts, n]: grp float64 running sums over slices g, g + grp, ..., then ((s0 + s1) + s2) + ..."""
    p64 = part.astype(np.float64)
    total = None
    for g in range(grp):
        s = np.zeros(part.shape[1], dtype=np.float64)
        for j in range(g, part.shape[0], grp):
            s = s + p64[j]
        total = s if total is None else total + s
    return total


def wave_sum(part):
    """per column of part [parts, n]: 64 float64 lane sums over l, l + 64, ..., then the xor butterfly 32, 16, ..., 1 as lane 0 sees it"""
    p64 = part.astype(np.float64)
    v = np.zeros((64, part.shape[1]), dtype=np.float64)
    for b in range(part.shape[0]):
        v[b % 64] = v[b % 64] + p64[b]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ o]
    return v[0]


def test_wgrad_group_vector_sum_order():
    from cmr_agent_amd import ops
    rng = np.random.default_rng(20240)
    for nparts in (1, 3, 4, 5, 31, 32, 33, 100):          # around one slice group (4) and around groups x loads in flight (32)
        for ln in (1, 33, 64, 65):                        # 2 len outputs: less than, exactly and more than a 64-output block
            plain = mixed(rng, (nparts, 2 * ln))
            old = mixed(rng, (2 * ln,))
            for part, acc in [(p, a) for p in ([plain, plant_pairs(rng, plain)] if nparts > 1 else [plain]) for a in (False, True)]:
                want64 = slice_group_sum(part, 4)
                (check_is_the_sum if part is plain else check_rounded_sum)(want64, part)
                want = want64.astype(np.float32)
                if acc:
                    want = old + want                       # fp32 addition to the old value
                got = []
                for _ in range(2):
                    oa, ob = torch.from_numpy(old[:ln].copy()).to(DEV), torch.from_numpy(old[ln:].copy()).to(DEV)
                    ops.wgrad_group((), vectors=[(torch.from_numpy(part).to(DEV), oa, ob, acc)])
                    got.append(np.concatenate([oa.cpu().numpy(), ob.cpu().numpy()]))
                assert np.array_equal(bits(got[0]), bits(want)), (nparts, ln, acc, part is plain)
                assert np.array_equal(bits(got[0]), bits(got[1])), (nparts, ln, acc, part is plain)


def test_bn_bwd_from_sums_wave_sum_order():
    from cmr_agent_amd import ops
    rng = np.random.default_rng(20241)
    rows, C = 32, 4                                        # C = 4: the smallest width the entry point accepts
    dz, x = (torch.from_numpy(mixed(rng, (rows, C))).to(DEV) for _ in range(2))
    stat = torch.from_numpy(np.abs(mixed(rng, (4, C)))).to(DEV)
    for parts in (1, 63, 64, 65, 200):                     # around one wave of lanes, and several partials per lane
        plain = mixed(rng, (parts, 2 * C))               # [parts][2][C]
        for part in ([plain, plant_pairs(rng, plain)] if parts > 1 else [plain]):
            want64 = wave_sum(part)
            (check_is_the_sum if part is plain else check_rounded_sum)(want64, part)
            want = want64.astype(np.float32)               # [0:C] = sums of d -> dbeta, [C:2C] = sums of d xhat -> dgamma
            got = []
            for _ in range(2):
                dgamma, dbeta = (torch.full((C,), float("nan"), device=DEV) for _ in range(2))
                ops.bn_bwd_from_sums(dz, 0.2, x, stat, torch.from_numpy(part.reshape(parts, 2, C)).to(DEV), dgamma, dbeta)
                got.append(np.concatenate([dbeta.cpu().numpy(), dgamma.cpu().numpy()]))
            assert np.array_equal(bits(got[0]), bits(want)), (parts, part is plain)
            assert np.array_equal(bits(got[0]), bits(got[1])), (parts, part is plain)
