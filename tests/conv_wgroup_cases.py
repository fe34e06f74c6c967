"""Cases of tests/test_conv_wgroup.py (CPU) and tests/test_conv_wgroup_gpu.py
(csrc/kernels/conv_wgroup.hip: the 3x3 forward, data gradient and weight gradient at Cg == Kg == 32).

The oracle, the inputs and the bounds are those of tests/conv_grouped_cases.py, which take any
``(N, H, W, C, Cg, sh, sw, ph, pw)``: forward and data gradient ``2^-8 |ref| + c T 2^-24 A`` with
``T = 9 Cg + 1 = 289`` terms, weight and bias gradient ``c' (M + 1) 2^-24 S``, ``c = c' = 1.01``.
The constants were checked on the path these kernels replace (SN_FEATURES=conv_wgroup=0: the
implicit grouped GEMM, its stride-2 data gradient through an fp32 dcol and col2im), not on the
kernels: MEASURED_PARENT_RATIOS holds the worst |got - ref| / bound that path reached over the cases
below with c = c' = 1.
"""
CASES = (
    (1, 1, 1, 32, 32, 1, 1, 1, 1),     # only the centre tap is in range
    (2, 2, 2, 32, 32, 2, 2, 1, 1),     # 2x2 at stride 2: phases with one tap, output 1x1
    (2, 7, 7, 64, 32, 1, 1, 1, 1),     # two groups; the 7x7 image of stage 5, a ragged tile
    (2, 8, 8, 64, 32, 2, 2, 1, 1),     # all four phases
    (2, 7, 7, 32, 32, 2, 2, 1, 1),     # odd size at stride 2: ragged last phase row and column
    (2, 9, 8, 32, 32, 2, 1, 0, 1),     # strides differ, pad 0 on one axis
    (1, 5, 7, 32, 32, 1, 1, 0, 0),     # pad 0, 15 output pixels
    (2, 6, 6, 32, 32, 1, 1, 2, 2),     # pad 2: output larger than input
    (1, 4, 4, 256, 32, 1, 1, 1, 1),    # eight groups: more than one block
    (5, 33, 17, 32, 32, 1, 1, 1, 1),   # several weight-gradient slabs, ragged last tile
)
LARGEST = CASES[-1]
IDS = ["x".join(map(str, c)) for c in CASES]

# worst |got - ref| / bound of the conv_wgroup=0 path with c = c' = 1 over CASES
MEASURED_PARENT_RATIOS = {"forward": 0.972, "dgrad": 0.982, "wgrad": 0.406, "bgrad": 0.021}  # all below 1: 1.01 stays
