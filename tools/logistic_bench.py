#!/usr/bin/env python3
"""Case / control association scan at cohort shape: GenotypeStore.assoc_logistic on the input of tools/grm_bench.py (a
2504-sample cohort file with one chr1-sized group, 230 k synthetic variants, converter output in /dev/shm), all samples, 10
covariates (11 columns of X and the dosage) and one 0 / 1 phenotype with a planted effect at variant PLANTED.

Reports, as one JSON line and in profiles/logistic_bench.json: the call's ms cold (every chunk read from the file and
uploaded) and with every chunk in the read cache, for test = "wald" (hhgt_logistic_fit) and test = "score" (hhgt_assoc_sums);
the kernel ms of the Wald call's stages (ctx.profile_read(): "decode" holds hhgt_genotype_planes, "ld_transpose"
hhgt_variant_planes, "assoc" hhgt_logistic_fit), the mean Newton steps per fitted variant and the status counts; and,
alternating with it repetition by repetition in the same warmed-up process, the torch route on the cached chunks:
read_windows of every sample, a float64 dosage matrix [V, S] with the calls that are not complete imputed to the variant's
mean, and the same Newton iteration batched over slices of TORCH_SLICE variants — the information matrix from three matmuls
against the per-sample products of X's columns, torch.linalg.cholesky, the same stopping rule, converged variants frozen.
Medians of the runs and every run; the first repetition is printed but kept out of the medians.  Before any time is taken
the two routes are compared: the same variants fitted, and the largest difference of BETA and SE relative to
max(|value|, 1e-3), asserted below 1e-6.  Not timed: building and converting the cohort, the design on the host, the warm-up.
usage: logistic_bench.py [variants] [runs]"""
import os, shutil, sys, tempfile
import numpy as np
import torch
from cohort_bench import build_cohort, report, summarize, timed
from haplohyped_varawareml_amd import device as dev
from haplohyped_varawareml_amd.store import (LOGIT_BETA, LOGIT_NOT_CONVERGED, LOGIT_P, LOGIT_SE, LOGIT_STATUS_NAMES, LOGIT_TESTED,
                                             GenotypeStore, logistic_design)

V = int(sys.argv[1]) if len(sys.argv) > 1 else 230_000
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
S, SEED, G = 2504, 1001, "chr_1"
BIG = 1 << 40
COVARIATES = 10
PLANTED = 1234 % V
TORCH_SLICE = 8192


def dosages(st):
    """read_windows of every sample (slices of 256) -> (the float64 dosages [V, S], 0 where a call is not complete, and
    which calls are complete, bool [V, S])"""
    device = st._context().device
    D = torch.empty((V, S), dtype=torch.float64, device=device)
    M = torch.empty((V, S), dtype=torch.bool, device=device)
    for i in range(0, S, 256):
        x = torch.stack(st.read_windows([(G, s, 0, V) for s in range(i, min(i + 256, S))]))   # [n, V, 2] int8
        a, b = x[..., 0], x[..., 1]
        done = ((a == 0) | (a == 1)) & ((b == 0) | (b == 1))
        D[:, i:i + x.shape[0]] = torch.where(done, (a + b).double(), torch.zeros((), dtype=torch.float64, device=device)).T
        M[:, i:i + x.shape[0]] = done.T
    return D, M


def torch_route(st, X, y, beta0):
    """the dosages, imputed, and the batched Newton iteration of store.logistic_fit_reference -> (beta, se, status, steps),
    [V] each: status LOGIT_TESTED or LOGIT_NOT_CONVERGED where the variant has two classes of calls, -1 elsewhere"""
    D, M = dosages(st)
    device = D.device
    X, y, beta0 = (torch.from_numpy(t).to(device) for t in (X, y, beta0))
    q = X.shape[1]
    XX = (X[:, :, None] * X[:, None, :]).reshape(S, q * q)
    m = M.sum(1).double()
    D = torch.where(M, D, (D.sum(1) / m)[:, None])
    classes = ((D == 0) & M).any(1).long() + ((D == 1) & M).any(1).long() + ((D == 2) & M).any(1).long()
    beta = torch.full((V,), float("nan"), dtype=torch.float64, device=device)
    se, status, steps = beta.clone(), torch.full((V,), -1, device=device), torch.zeros(V, dtype=torch.int64, device=device)
    for v0 in range(0, V, TORCH_SLICE):
        g = D[v0:v0 + TORCH_SLICE]
        n = g.shape[0]
        theta = torch.cat([beta0.expand(n, q), torch.zeros((n, 1), dtype=torch.float64, device=device)], 1)
        live = (m[v0:v0 + n] > 0) & (classes[v0:v0 + n] >= 2)
        last = torch.zeros(n, dtype=torch.bool, device=device)
        lost, count, hinv = last.clone(), torch.zeros(n, dtype=torch.int64, device=device), theta[:, 0] * float("nan")
        H = torch.empty((n, q + 1, q + 1), dtype=torch.float64, device=device)
        for _ in range(26):
            mu = torch.sigmoid(theta[:, :q] @ X.T + theta[:, q:] * g)
            w, r = mu * (1.0 - mu), y[None, :] - mu
            wg = w * g
            H[:, :q, :q] = (w @ XX).reshape(n, q, q)
            H[:, :q, q] = H[:, q, :q] = wg @ X
            H[:, q, q] = (wg * g).sum(1)
            U = torch.cat([r @ X, (r * g).sum(1, keepdim=True)], 1)
            L, bad = torch.linalg.cholesky_ex(H)
            delta = torch.cholesky_solve(U[:, :, None], L)[:, :, 0]
            ok = (bad == 0) & torch.isfinite(delta).all(1)
            lost |= live & ~ok
            hinv = torch.where(live & last & ok, 1.0 / (L[:, q, q] * L[:, q, q]), hinv)
            step = live & ~last & ok
            live = step.clone()
            theta = torch.where(step[:, None], theta + delta, theta)
            count += step
            small = delta.abs().amax(1) <= 1e-8
            last |= step & small
            lost |= step & ~small & (count == 25)
            live &= ~(lost)
            if not bool(live.any()):
                break
        done = last & ~lost & ~torch.isnan(hinv)
        beta[v0:v0 + n] = torch.where(done, theta[:, q], beta[v0:v0 + n])
        se[v0:v0 + n] = torch.where(done, hinv ** 0.5, se[v0:v0 + n])
        two = (m[v0:v0 + n] > 0) & (classes[v0:v0 + n] >= 2)
        status[v0:v0 + n] = torch.where(two, torch.where(done, LOGIT_TESTED, LOGIT_NOT_CONVERGED), -1)
        steps[v0:v0 + n] = count
    return beta, se, status, steps


tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    ctx = dev.Context(0)
    h5 = build_cohort(ctx, tmp, V, S, SEED)
    ctx.profile(True)
    warm = GenotypeStore(h5, ctx=ctx, cache_bytes=BIG)
    rng = np.random.default_rng(SEED)
    cov = rng.normal(size=(S, COVARIATES))
    planted = torch.stack(warm.read_windows([(G, s, PLANTED, PLANTED + 1) for s in range(S)]))[:, 0].clamp(min=0).sum(1).cpu().numpy()
    eta = 0.4 * (planted - planted.mean()) + 0.5 * cov[:, 0] - 0.7
    y = (rng.random(S) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    X, beta0 = logistic_design(y, cov)
    out = dict(samples=S, variants=V, runs=RUNS, covariates=COVARIATES, phenotypes=1, columns=int(X.shape[1]) + 1,
               cases=int(y.sum()), planted=PLANTED)

    # correctness first, which is also the warm-up of both routes (code objects loaded, the allocator grown)
    t_beta, t_se, t_status, _ = torch_route(warm, X, y, beta0)
    stats, calls, info = warm.assoc_logistic(G, y, cov)
    status = info[:, 0, 1]
    fitted = status == LOGIT_TESTED
    assert torch.equal(fitted, t_status == LOGIT_TESTED) and torch.equal(status == LOGIT_NOT_CONVERGED, t_status == LOGIT_NOT_CONVERGED)
    rel = max(float(((stats[:, 0, c] - t)[fitted].abs() / t[fitted].abs().clamp(min=1e-3)).max())
              for c, t in ((LOGIT_BETA, t_beta), (LOGIT_SE, t_se)))
    assert rel < 1e-6, rel
    p = torch.nan_to_num(stats[:, 0, LOGIT_P], nan=1.0)
    out.update(same_variants_fitted=True, largest_relative_difference=rel, smallest_p=float(p.min()),
               planted_has_smallest_p=int(p.argmin()) == PLANTED,
               status_counts={LOGIT_STATUS_NAMES[k].replace(" ", "_"): int((status == k).sum()) for k in range(5)},
               mean_steps_per_fitted_variant=float(info[:, 0, 0][fitted].double().mean()))
    del t_beta, t_se, t_status, stats, calls, info, status, fitted, p

    cold = GenotypeStore(h5, ctx=ctx)
    runs = dict(wald_cold_ms=[], wald_cached_ms=[], score_cold_ms=[], score_cached_ms=[], planes_kernel_ms=[],
                transpose_kernel_ms=[], logistic_kernel_ms=[], score_sums_kernel_ms=[], torch_cached_ms=[])
    for _ in range(RUNS + 1):
        runs["wald_cold_ms"].append(timed(lambda: cold.assoc_logistic(G, y, cov))[1])
        runs["torch_cached_ms"].append(timed(lambda: torch_route(warm, X, y, beta0))[1])
        ctx.profile_reset()
        runs["wald_cached_ms"].append(timed(lambda: warm.assoc_logistic(G, y, cov))[1])
        prof = ctx.profile_read()
        runs["planes_kernel_ms"].append(prof["decode"]["ms"])
        runs["transpose_kernel_ms"].append(prof["ld_transpose"]["ms"])
        runs["logistic_kernel_ms"].append(prof["assoc"]["ms"])
        runs["score_cold_ms"].append(timed(lambda: cold.assoc_logistic(G, y, cov, test="score"))[1])
        ctx.profile_reset()
        runs["score_cached_ms"].append(timed(lambda: warm.assoc_logistic(G, y, cov, test="score"))[1])
        runs["score_sums_kernel_ms"].append(ctx.profile_read()["assoc"]["ms"])
    medians, spreads = summarize(runs)                  # (of every repetition but the first)
    out.update(runs_ms=runs, **medians, **spreads)
    out.update(wald_cached_vs_torch_cached=out["wald_cached_ms"] / out["torch_cached_ms"])
    warm.close()
    cold.close()
    report("logistic_bench", out)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
