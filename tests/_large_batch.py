"""The cases of the large-batch regime (B > 256: the two-launch draw, steps
whose head and slab reduce leave the draw counter alone, the side-stream
prefetch, every exchange's B > 256 branch), shared by tests/test_large_batch.py
(the restatement alone, on the CPU) and tests/test_gpu_large_batch.py.

A draw is (seed, ctr) on a ring (capacity, lanes, head, valid per lane, n); the
device must reproduce tests/_nstep_ref.draw for every one listed here, so every
one is first checked to be a legal set the restatement finds within ROUND_CAP
rounds -- well inside the kernel's kDrawRounds = 4096.
"""
SEED = 13
DRAWS = 6
ROUND_CAP = 1024

# (B, capacity, lanes, head, valid per lane, n)
DRAW_CASES = [
    (257, 600, 1, 57, 600, 1),       # one over the boundary
    (384, 1000, 1, 0, 1000, 1),      # head 0: nothing forbidden
    (1000, 2500, 1, 123, 2500, 1),   # 1024 threads, B < P2
    (1024, 1100, 1, 5, 1100, 1),     # B == P2, many redraw rounds
    (300, 301, 1, 7, 301, 1),        # every allowed slot drawn: the redraw loop's long tail
    (264, 360, 3, 2, 110, 3),        # laned, n-step forbidden windows
    (320, 900, 1, 5, 900, 3),        # n-step, plain ring
]


def case_id(c):
    return "B%d-cap%d-lanes%d-n%d" % (c[0], c[1], c[2], c[5])


# The step tests' rings: N slots, all filled.
N, N1024 = 700, 2100
MODES_HEAD, MODES_SEED, MODES_STEPS = 5, 11, 11          # 1b
SWITCH_SEED, SWITCH_STEPS = 5, 20                        # 1c
TEACHER_SEED = 1234                                      # 1d
# (S, B, ring slots, rule, lr, steps)
TEACHER_CASES = [(16, 264, N, "rmsprop", 1e-4, 4), (24, 288, N, "sgd", 1e-2, 2),
                 (16, 1024, N1024, "sgd", 1e-2, 1)]
EXCHANGE_B = 264

# Every device draw the step tests make: (what, seed, first ctr, draws, B,
# capacity, lanes, head, valid, n).  The groups' members draw the same sets from
# rings of their own; an async worker draws once at the start and once a tick.
CHAINS = [
    ("modes S16 n1", MODES_SEED, 0, MODES_STEPS, 264, N, 1, MODES_HEAD, N, 1),
    ("modes S16 n3", MODES_SEED, 0, MODES_STEPS, 264, N, 1, MODES_HEAD, N, 3),
    ("modes S24 n1", MODES_SEED, 0, MODES_STEPS, 288, N, 1, MODES_HEAD, N, 1),
    ("modes S24 n3", MODES_SEED, 0, MODES_STEPS, 288, N, 1, MODES_HEAD, N, 3),
    ("switch", SWITCH_SEED, 0, SWITCH_STEPS, 264, N, 1, 0, N, 1),
    ("teacher 264", TEACHER_SEED, 0, 4, 264, N, 1, 0, N, 1),
    ("teacher 288", TEACHER_SEED, 0, 2, 288, N, 1, 0, N, 1),
    ("teacher 1024", TEACHER_SEED, 0, 1, 1024, N1024, 1, 0, N1024, 1),
    ("one-member allreduce", 9, 0, 14, EXCHANGE_B, N, 1, 0, N, 1),
    ("group step 0", 40, 0, 1, EXCHANGE_B, N, 1, 0, N, 1),
    ("group step 1", 41, 1, 1, EXCHANGE_B, N, 1, 0, N, 1),
    ("group async", 5, 0, 4, EXCHANGE_B, N, 1, 0, N, 1),
    ("rccl world 1", 9, 0, 18, EXCHANGE_B, N, 1, 0, N, 1),
    ("rccl world 1 async", 9, 0, 14, EXCHANGE_B, N, 1, 0, N, 1),
    ("monitor", 5, 0, 3, 300, N, 1, 0, N, 1),
]
