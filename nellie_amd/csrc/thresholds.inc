// Part of libnellie_hip.so: included by nellie_sample.hip and nellie_hip.hip (host code).
// =================================================================================================
// Histogram thresholds of nellie/utils/gpu_functions.py:23-94 on a finished histogram
// =================================================================================================
// The device builds the histogram (sampling.inc); what is left are a few hundred float64 operations on `nbins` counts.
// They run here, on the host, in C++: the results have to carry numpy's bits, and numpy evaluates `peak ** 2` of the
// triangle construction with libm's pow() -- the same libm this library links.  Every array expression of the
// reference is one left-to-right loop below (numpy's cumsum is a plain running sum; `x / y` on int64 operands is a
// float64 division of the converted values; the bin centres are float32: (e[i] + e[i+1]) / 2 in float32).
//
//   otsu     : centre of the bin that maximises the between-class variance w1 w2 (m1 - m2)^2        :36-50
//   triangle : centre of the bin farthest from the chord (first non-empty bin) -> (histogram peak),
//              walked from the longer tail (the histogram is mirrored when the peak sits nearer the low end)   :64-94
#include <cmath>
#include <vector>

// numpy's argmax on float64: a NaN is the maximum, the first one wins; otherwise the first largest value
static int np_argmax_f64(const double *a, int n) {
    double best = a[0];
    int at = 0;
    if (std::isnan(best)) return 0;
    for (int i = 1; i < n; ++i)
        if (!(a[i] <= best)) {
            best = a[i]; at = i;
            if (std::isnan(best)) break;
        }
    return at;
}

// status: 0 both thresholds valid; 1 the triangle construction is degenerate (the reference raises numpy's
// "attempt to get argmax of an empty sequence": peak, first and last non-empty bin coincide)
// EDGE = float for float32 data (numpy builds float32 edges and float32 centres for them), double for integer and float64
// data (the intensity thresholds of Label on the original image: float64 edges, float64 centres).  *otsu_var (may be NULL)
// = the between-class variance at the threshold, the second value gpu_functions.py:50 returns.
template <typename EDGE>
static void hist_thresholds_host(const int64_t *counts, const EDGE *edges, int nbins, double *triangle, double *otsu, int *status,
                                 double *otsu_var = nullptr) {
    std::vector<double> p(nbins), w1(nbins), w2(nbins), m1(nbins), m2(nbins), pc(nbins);
    std::vector<EDGE> centre(nbins);
    int64_t total = 0;
    for (int i = 0; i < nbins; ++i) total += counts[i];
    for (int i = 0; i < nbins; ++i) {
        centre[i] = (edges[i] + edges[i + 1]) / (EDGE)2;
        p[i] = (double)counts[i] / (double)total;
        pc[i] = p[i] * (double)centre[i];
    }
    // ---- Otsu: class weights and means from both ends
    {
        double acc = 0.0, accm = 0.0;
        for (int i = 0; i < nbins; ++i) { acc += p[i]; accm += pc[i]; w1[i] = acc; m1[i] = accm / acc; }
        acc = 0.0; accm = 0.0;
        for (int i = nbins - 1; i >= 0; --i) { acc += p[i]; accm += pc[i]; w2[i] = acc; m2[i] = accm / acc; }
        if (nbins < 2) { *otsu = (double)centre[0]; if (otsu_var) *otsu_var = 0.0; }
        else {
            std::vector<double> var(nbins - 1);
            for (int i = 0; i + 1 < nbins; ++i) {
                const double d = m1[i] - m2[i + 1];
                var[i] = (w1[i] * w2[i + 1]) * (d * d);
            }
            const int at = np_argmax_f64(var.data(), nbins - 1);
            *otsu = (double)centre[at];
            if (otsu_var) *otsu_var = var[at];
        }
    }
    // ---- triangle
    *status = 0;
    int peak = np_argmax_f64(p.data(), nbins);
    double height = p[peak];
    int lo = -1, hi = -1;
    for (int i = 0; i < nbins; ++i)
        if (p[i] != 0.0) { if (lo < 0) lo = i; hi = i; }
    const bool mirrored = (peak - lo) < (hi - peak);
    if (mirrored) { lo = nbins - hi - 1; peak = nbins - peak - 1; }
    const int span = peak - lo;
    if (span <= 0 || lo < 0) { *status = 1; *triangle = 0.0; return; }
    const double norm = std::sqrt(std::pow(height, 2.0) + (double)((int64_t)span * (int64_t)span));
    const double hn = height / norm, sn = (double)span / norm;
    std::vector<double> dist(span);
    for (int k = 0; k < span; ++k) {
        const int bin = mirrored ? nbins - 1 - (k + lo) : k + lo;        // the k-th bin of the (mirrored) walk
        dist[k] = hn * (double)k - sn * p[bin];
    }
    int level = np_argmax_f64(dist.data(), span) + lo;
    if (mirrored) level = nbins - level - 1;
    *triangle = (double)centre[level];
}
