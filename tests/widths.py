"""The feature widths at which the GPU tests launch every built copy of the fused loss kernels.  No device code, and no GPU
test module, is imported here; tests/test_width_coverage.py holds the lists to the sources' MAX_NDT / MAX_NK / MAX_NF.

idg_mixnce.hip, idg_sccf.hip, idg_nance.hip and idg_svdnce.hip instantiate their tile kernels per NDT = ceil(d / 32), 1 .. 8;
idg_vae.hip's matrix-core form per NK = d / 32, 1 .. 8; idg_au.hip's per NF = d / 64, 1 .. 4.  OLD_GRID names, per source, the
widths its GPU file ran on those kernels before these lists existed."""

# NDT 1, 3, 3, 4, 5, 5, 6, 7, 7, 8.  72, 130 and 200 are no multiple of 32: padding columns in three of the NDT values the old
# grids never reached; 256 is there again so that the same cases run the rolled chunk loop's far end
EVERY_NDT = (32, 72, 96, 128, 130, 160, 192, 200, 224, 256)

# multiples of 32 (the matrix-core forms of idg_vae.hip and idg_au.hip take no other width): NK 3, 5, 6, 7; 192 is NF 3
EVERY_NK = (96, 160, 192, 224)
NF3_WIDTH = 192

# LightGCL's second row per width (B = 300, N = 1000, q = 16: several table chunks and query splits)
LIGHTGCL_CHUNKED = (96, 128, 160, 224)

B_TILES = (129, 257)  # two 128-row tiles with one live row in the second; a third tile and a non-trivial chunk split

# the widths each source's width-templated kernels were launched at by the older cases of its GPU file (LightGCL: those of
# its GRID with B > SMALL_B = 127 only — the rows below take the direct form, which has no NDT)
OLD_GRID = {
    "idg_mixnce.hip": (48, 64, 100, 256),
    "idg_sccf.hip": (48, 64, 100, 256),
    "idg_nance.hip": (48, 64, 100, 256),
    "idg_svdnce.hip": (32, 48, 64, 256),
    "idg_vae.hip": (32, 64, 128, 256),
    "idg_au.hip": (64, 128, 256),
}


def ndt(d):
    return (d + 31) // 32
