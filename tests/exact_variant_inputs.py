"""Shapes of the tests that run exact kNN's option-selected kernels and its forced small tables (tests/test_gpu_exact_variants.py;
tests/test_exact_variant_inputs_cpu.py proves the claims), and the host plans those tests reason from, restated in Python:
filter_plan_k (csrc/exact_host.h) and the walk of exf_wide_filter_kernel over strips, segments and rounds (csrc/exact_wide.h).
Nothing here touches a device."""
import collections

EXF_SAMPLE = 32768            # exact2.h: rows of the threshold sample
EXF_K_SAMPLE_MAX, EXF_K_CAP_FACTOR = 8, 4   # exact_host.h
EXF_PF = 4                    # exact2.h: k-steps a wave keeps in flight
WAVES = 8                     # exact2.h: EXF_WG / 64

FilterPlan = collections.namedtuple("FilterPlan", "n_sample sample_stride cap")


def filter_plan_k(N, k, refine_all=False):
    """exact_host.h filter_plan_k (k <= 32: filter_plan), field for field"""
    full_strips = N // 32
    want = EXF_SAMPLE * (min(EXF_K_SAMPLE_MAX, (k + 31) // 32) if k > 32 else 1)
    n_sample = min(full_strips, want // 32) * 32
    if k <= 32:
        cap = N if refine_all else min(N, 8192)
    else:
        per_sample_row = (N + n_sample - 1) // n_sample if n_sample > 0 else N
        cap = N if refine_all else min(N, max(8192, EXF_K_CAP_FACTOR * k * per_sample_row))
    return FilterPlan(n_sample, max(1, full_strips // (n_sample // 32)) if n_sample > 0 else 1, cap)


# ---- the wide shapes (option exact_wide_shape -> TS k-steps per segment, R strips per wave, workgroups per CU) ----------------
WIDE_SHAPES = {0: (8, 1, 2), 1: (16, 1, 1), 2: (8, 2, 1)}
WIDE_N = 8192 + 77
WIDE_DS = (516, 768, 2048)
WIDE_QS = (1, 9, 33, 70)
WIDE_GRID_CUS = (3, 4)        # 3: several rounds, the last with idle waves; 4: the last with idle workgroups under every shape


def segments(d, TS):
    """k-steps of each LDS segment of a row of d elements: T = ceil(d / 16) in pieces of TS, the last one short"""
    T = (d + 15) // 16
    return [min(TS, T - s) for s in range(0, T, TS)]


def wide_walk(N, shape, n_cus):
    """exf_wide_filter_kernel over N rows on n_cus CUs: (workgroups, rounds of workgroup 0, live strips per wave of the LAST
    workgroup-round that holds a strip, workgroups without a strip in the last round)"""
    TS, R, per_cu = WIDE_SHAPES[shape]
    strips = (N + 31) // 32
    per_wg = WAVES * R
    grid = max(1, min((strips + per_wg - 1) // per_wg, n_cus * per_cu))
    rounds = (strips - 0 + grid * per_wg - 1) // (grid * per_wg)
    last_first = ((strips - 1) // per_wg) * per_wg                         # the first strip of the last workgroup-round with work
    live = [max(0, min(R, strips - (last_first + w * R))) for w in range(WAVES)]
    last_round_wgs = (strips - (rounds - 1) * grid * per_wg + per_wg - 1) // per_wg
    return grid, rounds, live, grid - last_round_wgs


# ---- forced small tables at k > 32 (exact_filter = 1, exact_filter_k = 1024): (N, k, what it reaches) ------------------------
SMALL_TABLES = (
    (2080, 1024, "the sample equals the table"),
    (1000, 1024, "992 sample rows are fewer than k"),
    (1000, 512, "992 sample rows are more than k"),
    (300, 512, "fewer rows than k: padding behind the tree merge"),
    (31, 40, "no full strip"),
    (3, 64, "a table of three rows"),
)
SMALL_WIDE = tuple(t for t in SMALL_TABLES if t[0] in (1000, 31))
