// Host-side utilities of libemdenoise.so (no GPU work): CRC-32C for the TFRecord reader, the box-resize table of the harvester.
// TFRecord framing (the container misc_py/TFRecord_creator.py:57-85 writes through
// tf.python_io.TFRecordWriter): uint64 length | masked crc32c(length) | data | masked crc32c(data).
#include <nmmintrin.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace emd {
void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));   // emd_common.hip
}

extern "C" uint32_t emd_crc32c(const void* data_host, size_t n, uint32_t crc) {
    const unsigned char* p = static_cast<const unsigned char*>(data_host);
    uint64_t c = crc ^ 0xffffffffu;
    while (n && (reinterpret_cast<uintptr_t>(p) & 7)) {
        c = _mm_crc32_u8((uint32_t)c, *p++);
        --n;
    }
    while (n >= 8) {
        uint64_t v;
        std::memcpy(&v, p, 8);
        c = _mm_crc32_u64(c, v);
        p += 8;
        n -= 8;
    }
    while (n--) c = _mm_crc32_u8((uint32_t)c, *p++);
    return (uint32_t)c ^ 0xffffffffu;
}

// The member runs of MATLAB's imresize(..., 'method', 'box') with antialiasing, n_in -> n_out samples along one axis
// (include/emdenoise.h has the expressions; images.internal.resize's contributions() for the box kernel).  Every product, quotient
// and sum rounds on its own: a fused multiply-add would move the ties.
#pragma clang fp contract(off)
extern "C" int emd_box_resize_table(int n_in, int n_out, int* tab) {
    if (!tab) {
        emd::set_error("emd_box_resize_table: null pointer");
        return -1;
    }
    if (n_in < 1 || n_in > 32768 || n_out < 1 || n_out > 8192) {
        emd::set_error("emd_box_resize_table: 1 <= n_in <= 32768 and 1 <= n_out <= 8192 (got %d -> %d)", n_in, n_out);
        return -1;
    }
    const double scale = (double)n_out / (double)n_in;
    const bool shrink = scale < 1.0;
    const double kw = shrink ? 1.0 / scale : 1.0;
    const int ncand = (int)std::ceil(kw) + 2;
    for (int x = 1; x <= n_out; ++x) {
        const double u = (double)x / scale + 0.5 * (1.0 - 1.0 / scale);
        const long left = (long)std::floor(u - kw / 2.0);
        long first = 0, last = 0;
        int count = 0;
        for (int k = 0; k < ncand; ++k) {
            const long i = left + k;
            const double diff = u - (double)i;
            const double t = shrink ? scale * diff : diff;
            if (-0.5 <= t && t < 0.5) {
                if (!count) first = i;
                last = i;
                ++count;
            }
        }
        // one contiguous, non-empty run inside 1..n_in (so the mirror fold of indices never applies): holds for every size pair
        // tried; a pair where it did not would need the general weights
        if (!count || last - first + 1 != count || first < 1 || last > n_in) {
            emd::set_error("emd_box_resize_table: output %d of %d -> %d has no contiguous run of members inside the input", x, n_in, n_out);
            return -2;
        }
        tab[2 * (x - 1)] = (int)(first - 1);
        tab[2 * (x - 1) + 1] = count;
    }
    return 0;
}
