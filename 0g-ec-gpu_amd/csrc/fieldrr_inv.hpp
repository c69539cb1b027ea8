// Field inversion in the reduced-radix form (fieldrr.hpp), shared by the
// field-operation test entry (fieldops.hip) and the Fr scans (fr_scan.hip).
#pragma once
#include "fieldrr.hpp"

namespace ecg {

template <class Q>
ECG_DEV FpR<Q> rr_inv_fermat(const FpR<Q>& a) {  // a^(p-2), MSB first
  using P = typename Q::Base;
  FpR<Q> r = FpR<Q>::one();
  for (int i = P::N - 1; i >= 0; i--) {
    const uint64_t e = P::PM2[i];
    for (int bit = 63; bit >= 0; bit--) {
      r = rr_sqr(r);
      if ((e >> bit) & 1) r = rr_mul(r, a);
    }
  }
  return r;
}

}  // namespace ecg
