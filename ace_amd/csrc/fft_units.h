// Workgroup -> unit mappings and the 32-bit lane-offset bound of the two-level longitude FFT kernels (fft.hip).  Plain C++ shared by
// the kernels (device, called with blockIdx / gridDim), their launchers (host) and the CPU test (tests/emul/fft_units_emul.cpp).
#pragma once

#if defined(__HIPCC__)
#define FFTU_HD __host__ __device__ __forceinline__
#else
#define FFTU_HD inline
#endif

namespace ace {

// Workgroup -> (channel block, latitude).  Workgroups go round-robin over the 8 XCDs by linear id, and every XCD has its own L2:
// in launch order the R-row (64- or 128-byte) spectral runs of neighbouring channel blocks would be written from eight different
// L2s as partial lines.  With a unit count divisible by 8, XCD x takes the contiguous unit range [x T/8, (x+1) T/8) instead, so
// the channel blocks of one latitude share an L2 and leave it as whole lines.
// (r03 same-box A/B at 1 degree: forward 71.7 -> 68.0 us; the inverse kernel, whose spectral side is READ in 128-byte runs,
// got slower, 54.6 -> 59.1 us, and keeps launch order.)
// id = blockIdx.x + gx * blockIdx.y, gx = gridDim.x (channel blocks), gy = gridDim.y (latitudes)
template <bool XCD>
FFTU_HD void fft_unit(const int id, const int gx, const int gy, int& cblk, int& lat) {
    const int total = gx * gy;
    int u = id;
    if (XCD && (total & 7) == 0) u = (id & 7) * (total >> 3) + (id >> 3);
    cblk = u % gx;
    lat = u / gx;
}
// The forward kernel's form with RIDER workgroups (DftArgs::nride, pack_frag.h): the grid's y extent carries ceil(nride / gx) extra
// rows; the riders are the FIRST units of every XCD's range - dispatched first, their slots go back to the transform's own
// workgroups (at the end they would sit in the launch's tail; all on one XCD they cost its range 2 us).  Returns true for a rider
// (index rid, idle when rid >= nride).
template <bool XCD>
FFTU_HD bool fft_unit_ride(const int id, const int gx, const int gy, const int nride, int& cblk, int& lat, int& rid) {
    const int total = gx * gy;
    const int nextra = nride > 0 ? (nride + gx - 1) / gx * gx : 0;
    int u;
    if (XCD && (total & 7) == 0 && (nextra & 7) == 0) {
        const int xcd = id & 7, pos = id >> 3, nr8 = nextra >> 3;
        if (pos < nr8) { rid = pos * 8 + xcd; return true; }
        u = xcd * ((total >> 3) - nr8) + (pos - nr8);
    } else {
        if (id < nextra) { rid = id; return true; }
        u = id - nextra;
    }
    cblk = u % gx;
    lat = u / gx;
    return false;
}

// The kernels address with 32-bit lane offsets behind a buffer descriptor of 2^31 - 1 bytes: at most (N1 + 1) <= 41 spectral planes
// (H Bt 2 C floats each), and 32 grid rows, from a workgroup's base.  The planes input (P-format, [C/8][H W][8] halves per sample)
// is addressed from the SAMPLE's base with an absolute k-group: ((kg H W + w) 16) bytes, kg < C / 8 - up to 2 C H W bytes.  A launch
// beyond any of them would have its loads answered with zeros (stores dropped) by the descriptor's range check, silently: it does
// not take the FFT form.
FFTU_HD bool fft_lane_offsets_fit(const int H, const int W, const int Bt, const int C, const bool planes) {
    const double plane = (double)H * Bt * 2.0 * C * 4.0, rows = 33.0 * (double)H * W * 4.0;
    const double pln = planes ? 2.0 * (double)C * H * W : 0.0;
    return 42.0 * plane < 2147483647.0 && rows < 2147483647.0 && pln < 2147483647.0;
}

}  // namespace ace
