// Device resampler (srf_amd/resample.py): audio at any integer rate
// in [4000, 192000] Hz to another, Kaldi's LinearResample as ResampleWaveform configures
// it (cutoff 0.99 of the lower Nyquist frequency, 6 zeros, Hann-windowed sinc).  Output
// sample o = u ou + p (p its phase, iu / ou the reduced ratio) is the dot product of the
// phase's weight row with the inputs first[p] + u iu .. + taps - 1; inputs outside the
// signal are zero.  srf_resample_tables computes first and the weights on the host in
// double and rounds once; the kernel sums in fp32 in tap order with one fma per tap, so a
// sample's bits depend on its taps only, not on the launch, the tile or the chunking.
//
// resample_kernel: a workgroup owns `tile` consecutive outputs of one row.  It stages the
// tile's input span once in LDS as float (neighbouring outputs share all but iu / ou of
// their inputs) and then each thread runs the tap loop for its outputs.  Weights: a table
// of ou * (taps | 1) <= kWeightLdsFloats floats is staged in LDS too, its rows padded to an
// odd stride; a larger one (ou in the thousands: every output of a tile has a row of its
// own, there is nothing to share) is read from global memory, where a lane walks its own
// contiguous row.  No atomics, no workspace.
#include <algorithm>
#include <cmath>
#include <vector>

#include "srf_common.h"
#include "../../include/srf.h"

namespace {

constexpr int kMaxRates = SRF_RESAMPLE_MAX_RATES, kRateMin = 4000, kRateMax = 192000;
constexpr int kHdr0 = 8, kHdrStride = 8, kHeaderFloats = kHdr0 + kHdrStride * kMaxRates;
constexpr long long kMaxWeights = 1ll << 20;
constexpr int kThreads = 256;
constexpr int kWeightLdsFloats = 8192;     // a weight table up to 32 KB lives in LDS
constexpr int kLdsFloats = 16384;          // 64 KB of dynamic LDS per workgroup
constexpr int kMaxOut = 0x7fffffff - 2048; // o + tile stays an int
constexpr double kPi = 3.14159265358979323846;

struct Rate {
  int fin, fout, iu, ou;
  double fc, ww;   // cutoff (Hz) and half width (s) of the filter
};

int gcd_of(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

bool rate_ok(int r) { return r >= kRateMin && r <= kRateMax; }

Rate make_rate(int fin, int fout) {
  Rate r;
  const int g = gcd_of(fin, fout);
  r.fin = fin, r.fout = fout, r.iu = fin / g, r.ou = fout / g;
  r.fc = 0.99 * 0.5 * (fin < fout ? fin : fout);
  r.ww = 6.0 / (2.0 * r.fc);
  return r;
}

// first and last input index of phase p, relative to u * iu; equal rates copy
int first_of(const Rate& r, int p) {
  if (r.fin == r.fout) return 0;
  const double t = p / (double)r.fout;
  return (int)std::ceil((t - r.ww) * r.fin);
}
int last_of(const Rate& r, int p) {
  if (r.fin == r.fout) return 0;
  const double t = p / (double)r.fout;
  return (int)std::floor((t + r.ww) * r.fin);
}
int taps_of(const Rate& r) {
  int taps = 1;
  for (int p = 0; p < r.ou; ++p) taps = std::max(taps, last_of(r, p) - first_of(r, p) + 1);
  return taps;
}
// taps_of without the walk over the phases: floor(c + h) - ceil(c - h) + 1 <= 2 h + 1
int taps_bound(const Rate& r) { return r.fin == r.fout ? 1 : (int)std::floor(2.0 * r.ww * r.fin) + 2; }

double weight_of(const Rate& r, int p, int j) {
  if (r.fin == r.fout) return 1.0;
  const double t = p / (double)r.fout;
  const double d = (first_of(r, p) + j) / (double)r.fin - t;
  if (!(std::fabs(d) < r.ww)) return 0.0;
  const double win = 0.5 * (1.0 + std::cos(2.0 * kPi * r.fc / 6.0 * d));
  const double filt = d == 0.0 ? 2.0 * r.fc : std::sin(2.0 * kPi * r.fc * d) / (kPi * d);
  return win * filt / r.fin;
}

// validates a bank and returns its block size in floats, 0 with a message if refused
size_t bank_floats(const char* who, const int* rates_in, int n_rates, int rate_out, std::vector<int>* taps_out) {
  if (!rates_in || n_rates < 1 || n_rates > kMaxRates) {
    srf::set_error("%s: a bank holds 1 .. %d input rates, got %d", who, kMaxRates, n_rates);
    return 0;
  }
  if (!rate_ok(rate_out)) {
    srf::set_error("%s: the output rate %d lies outside [%d, %d] Hz", who, rate_out, kRateMin, kRateMax);
    return 0;
  }
  long long weights = 0, firsts = 0;
  for (int i = 0; i < n_rates; ++i) {
    if (!rate_ok(rates_in[i])) {
      srf::set_error("%s: input rate %d (entry %d) lies outside [%d, %d] Hz", who, rates_in[i], i, kRateMin, kRateMax);
      return 0;
    }
    const Rate r = make_rate(rates_in[i], rate_out);
    const int taps = taps_of(r);
    if (taps_out) taps_out->push_back(taps);
    weights += (long long)r.ou * taps;
    firsts += r.ou;
  }
  if (weights > kMaxWeights) {
    srf::set_error("%s: the bank's weight tables hold %lld floats, more than %lld", who, weights, kMaxWeights);
    return 0;
  }
  return (size_t)(kHeaderFloats + firsts + weights);
}

__global__ __launch_bounds__(kThreads) void resample_kernel(
    const void* __restrict__ samples, int is_int16, const int* __restrict__ n_samples, const int* __restrict__ choice,
    const float* __restrict__ tab, int n_rates, int stride, int s0, int n_limit, int o0, int o1, int tile, int span_cap,
    int w_cap, float* __restrict__ out, int stride_out, int q0, int* __restrict__ n_out) {
  extern __shared__ float lds[];
  float* xs = lds;              // the tile's input span, global samples lo .. lo + span - 1
  float* wl = lds + span_cap;   // the weight table, row stride taps | 1
  const int b = blockIdx.y, tid = threadIdx.x;
  const int ob = o0 + (int)blockIdx.x * tile, oe = min(ob + tile, o1);
  const int r = choice ? min(max(choice[b], 0), n_rates - 1) : 0;
  const float* h = tab + kHdr0 + kHdrStride * r;
  const int iu = (int)h[0], ou = (int)h[1], taps = (int)h[2];
  const float* first = tab + (int)h[3];
  const float* w = tab + (int)h[4];
  const int nb = min(max(n_samples[b], 0), n_limit);
  const long long lim = (long long)nb * ou;   // o < n_out(nb)  <=>  o iu < nb ou
  float* orow = out + (size_t)b * stride_out;
  if (n_out && blockIdx.x == 0 && tid == 0) n_out[b] = (int)min((lim + iu - 1) / iu, (long long)0x7fffffff);
  if ((long long)ob * iu >= lim) {   // the whole tile lies past the row's end
    for (int o = ob + tid; o < oe; o += kThreads) orow[o - q0] = 0.f;
    return;
  }
  // first[p] + u iu grows with o: the tile reads lo(ob) .. lo(oe - 1) + taps - 1
  const int ub = ob / ou, pb = ob - ub * ou, ue = (oe - 1) / ou, pe = oe - 1 - ue * ou;
  const long long lo = (long long)ub * iu + (int)first[pb];
  const int span = (int)((long long)ue * iu + (int)first[pe] + taps - lo);
  const int wstride = taps | 1;
  const bool w_lds = ou * wstride <= w_cap;
  if (span > span_cap) return;   // tables that were not built for the rates the launch was sized for
  for (int i = tid; i < span; i += kThreads) {
    const long long g = lo + i;
    float v = 0.f;
    if (g >= s0 && g < nb) {
      const size_t c = (size_t)b * stride + (size_t)(g - s0);
      v = is_int16 ? (float)static_cast<const short*>(samples)[c] : static_cast<const float*>(samples)[c];
    }
    xs[i] = v;
  }
  if (w_lds)
    for (int i = tid; i < ou * taps; i += kThreads) {
      const int p = i / taps;
      wl[p * wstride + (i - p * taps)] = w[i];
    }
  __syncthreads();
  for (int o = ob + tid; o < oe; o += kThreads) {
    float acc = 0.f;
    if ((long long)o * iu < lim) {
      const int u = o / ou, p = o - u * ou;
      const float* x = xs + (int)((long long)u * iu + (int)first[p] - lo);
      if (w_lds) {
        const float* wr = wl + p * wstride;
        for (int j = 0; j < taps; ++j) acc = fmaf(wr[j], x[j], acc);
      } else {
        const float* wr = w + (size_t)p * taps;
        for (int j = 0; j < taps; ++j) acc = fmaf(wr[j], x[j], acc);
      }
    }
    orow[o - q0] = acc;
  }
}

}  // namespace

extern "C" size_t srf_resample_table_floats(const int* rates_in, int n_rates, int rate_out) {
  return bank_floats("resample_table_floats", rates_in, n_rates, rate_out, nullptr);
}

extern "C" int srf_resample_tables(const int* rates_in, int n_rates, int rate_out, float* tables, size_t n_floats) {
  std::vector<int> taps;
  const size_t need = bank_floats("resample_tables", rates_in, n_rates, rate_out, &taps);
  if (!need) return SRF_EINVAL;
  SRF_REQUIRE(tables && n_floats >= need, "resample_tables: need a host buffer of %zu floats, got %zu", need, n_floats);
  for (int i = 0; i < kHeaderFloats; ++i) tables[i] = 0.f;
  tables[0] = (float)n_rates;
  tables[1] = (float)rate_out;
  size_t off = kHeaderFloats;
  for (int i = 0; i < n_rates; ++i) {
    const Rate r = make_rate(rates_in[i], rate_out);
    float* h = tables + kHdr0 + kHdrStride * i;
    const size_t off_first = off, off_w = off + r.ou;
    h[0] = (float)r.iu, h[1] = (float)r.ou, h[2] = (float)taps[i];
    h[3] = (float)off_first, h[4] = (float)off_w, h[5] = (float)r.fin;
    for (int p = 0; p < r.ou; ++p) {
      tables[off_first + p] = (float)first_of(r, p);
      for (int j = 0; j < taps[i]; ++j) tables[off_w + (size_t)p * taps[i] + j] = (float)weight_of(r, p, j);
    }
    off = off_w + (size_t)r.ou * taps[i];
  }
  return SRF_OK;
}

extern "C" size_t srf_resample_num_out(size_t n, int rate_in, int rate_out) {
  if (!rate_ok(rate_in) || !rate_ok(rate_out)) {
    srf::set_error("resample_num_out: rates %d -> %d outside [%d, %d] Hz", rate_in, rate_out, kRateMin, kRateMax);
    return 0;
  }
  const Rate r = make_rate(rate_in, rate_out);
  return (size_t)(((unsigned long long)n * (unsigned)r.ou + (unsigned)r.iu - 1) / (unsigned)r.iu);
}

extern "C" int srf_resample(const void* samples, int is_int16, const int* n_samples, const int* choice,
                            const float* tables, const int* rates_in, int n_rates, int rate_out, int B, int stride,
                            int width, int s0, int n_limit, int o0, int o1, float* out, int stride_out, int q0,
                            int* n_out, void* stream) {
  SRF_REQUIRE(B >= 1 && B <= 65535, "resample: need 1 <= B <= 65535 (B=%d)", B);
  SRF_REQUIRE(rates_in && n_rates >= 1 && n_rates <= kMaxRates, "resample: a bank holds 1 .. %d input rates, got %d",
              kMaxRates, n_rates);
  SRF_REQUIRE(rate_ok(rate_out), "resample: the output rate %d lies outside [%d, %d] Hz", rate_out, kRateMin, kRateMax);
  for (int i = 0; i < n_rates; ++i)
    SRF_REQUIRE(rate_ok(rates_in[i]), "resample: input rate %d (entry %d) lies outside [%d, %d] Hz", rates_in[i], i,
                kRateMin, kRateMax);
  SRF_REQUIRE(width >= 0 && stride >= width, "resample: need 0 <= width <= stride (width=%d stride=%d)", width, stride);
  SRF_REQUIRE(0 <= o0 && o0 <= o1 && o1 <= kMaxOut, "resample: bad output range [%d, %d)", o0, o1);
  if (o1 == o0) return SRF_OK;
  SRF_REQUIRE(samples && n_samples && tables && out, "resample: null pointer argument");
  SRF_REQUIRE(s0 >= 0 && n_limit >= 0 && (long long)n_limit <= (long long)s0 + width,
              "resample: n_limit %d lies beyond the buffer (samples %d .. %lld)", n_limit, s0, (long long)s0 + width);
  SRF_REQUIRE(stride_out >= 1 && o0 >= q0 && (long long)o1 - q0 <= stride_out,
              "resample: outputs [%d, %d) outside the output buffer (outputs %d .. %lld)", o0, o1, q0,
              (long long)q0 + stride_out);
  // size the tile for the bank: every rate's input span, and the largest weight table that goes to LDS
  int tile = 1024, span_cap = 0, w_cap = 0;
  for (;; tile >>= 1) {
    span_cap = w_cap = 0;
    for (int i = 0; i < n_rates; ++i) {
      const Rate r = make_rate(rates_in[i], rate_out);
      const int tb = taps_bound(r);
      // the first tap the launch reads: below s0 only where the signal has not begun
      const long long lo = (long long)(o0 / r.ou) * r.iu + first_of(r, o0 % r.ou);
      SRF_REQUIRE(s0 == 0 || lo >= s0, "resample: output %d of %d -> %d Hz reads sample %lld, before the buffer's first %d",
                  o0, r.fin, r.fout, lo, s0);
      span_cap = std::max(span_cap, (int)((long long)(tile - 1) * r.iu / r.ou) + tb + 2);
      const long long wf = (long long)r.ou * (tb | 1);
      if (wf <= kWeightLdsFloats) w_cap = std::max(w_cap, (int)wf);
    }
    if (span_cap + w_cap <= kLdsFloats || tile == 256) break;
  }
  if (span_cap + w_cap > kLdsFloats) w_cap = 0;   // a steep ratio with long rows: the span alone fits, weights from global
  const unsigned gx = (unsigned)((o1 - o0 + tile - 1) / tile);
  hipLaunchKernelGGL(resample_kernel, dim3(gx, (unsigned)B), dim3(kThreads), sizeof(float) * (size_t)(span_cap + w_cap),
                     static_cast<hipStream_t>(stream), samples, is_int16, n_samples, choice, tables, n_rates, stride, s0,
                     n_limit, o0, o1, tile, span_cap, w_cap, out, stride_out, q0, n_out);
  SRF_LAUNCH_CHECK("resample");
  return SRF_OK;
}
