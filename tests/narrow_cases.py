"""The case table of the 32-channel convolution tests (tests/test_conv_narrow_gpu.py on the device, tests/test_conv_narrow_ref.py on the
CPU): the two narrow 3 x 3 layers of the large_cnn front-end, (Cin, Cout) = (32, 32) pooled at level 0 and (32, 64) dense at level 1,
and conv0 with 32 output channels.  (kind, Cin, Cout, B, T, F) as in tests/conv_edge_util.CASES: Cin / Cout are the FORWARD
convolution's; the extents are those of the 64 / 128-channel table (odd sizes, no multiples of the 8 x 16 pixel tile, several tiles)."""

CASES = {
    'P32': ('pool', 32, 32, 2, 18, 21),
    'R64': ('relu', 32, 64, 2, 33, 20),
    'D32p': ('dgrad_p', 32, 32, 2, 17, 35),
    'D64d': ('dgrad_d', 32, 64, 1, 33, 20),
    'MANY32': ('pool', 32, 32, 8, 256, 80),       # 1280 pixel tiles: the persistent loop wraps
}
ONE = [('pool', 32, 32, 1, 2, 2), ('relu', 32, 64, 1, 1, 1), ('relu', 32, 64, 1, 1, 17), ('dgrad_d', 32, 64, 1, 1, 1), ('dgrad_d', 32, 64, 1, 1, 17)]
TASK_CASES = ('P32', 'R64', 'D32p', 'D64d')
STACKED = (('P32', 0), ('R64', 1), ('D32p', 0), ('D64d', 1))       # (case, wshift = the layer's resolution level)
WGRAD = [(32, 32, 2, 18, 21, True), (32, 64, 2, 17, 34, False), (32, 32, 1, 2, 2, True)]      # (Cin, Cout, B, T, F, pooled)
CONV0 = dict(B=2, T=(1, 5, 9), F=(1, 21), C=32)                   # T: no multiples of conv0's 4-frame tile
