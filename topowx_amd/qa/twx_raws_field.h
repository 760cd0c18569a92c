// twx_raws_field.h -- the token and field logic of the RAWS ingest (twxrw_raws.hip): what a token is, the grammar of the
// numbers the device decides, the date of token 0 and the three values of a line, as __host__ __device__ functions of
// bytes already in hand.  The kernels call them on the call's buffer; tests/tools/raws_hostcheck.cpp calls the same code
// on the CPU (g++, address and undefined-behaviour sanitizers).  Nothing here touches memory outside [s, s + n): every
// caller clips n to the line's own end first.
//
// Reference: InsertRaws.parse_stn_obs (twx/db/create_db_all_stations.py:1177-1233).  A token is what bytes.split() gives:
// a maximal run of bytes other than space, \t, \n, \v, \f, \r.  The device decides an int() field of the form
// [+-]?[0-9]{1,9} and a float() token of the form [+-]? digits with at most one '.', at least one digit, at most 15
// significant digits and at most 22 digits after the point; everything else is RW_UNCERTAIN and left to Python.
#ifndef TWX_RAWS_FIELD_H
#define TWX_RAWS_FIELD_H
#include <stdint.h>

#include "twx_ghcn_field.h"

#define RW_OK 0
#define RW_UNCERTAIN 1       // Python's int() / float() decides it

#define RW_TOK_MAX 40        // a field token longer than this is RW_UNCERTAIN
#define RW_MISSING (-9999.0)

#define RW_FIELD_DATE 0      // token 0
#define RW_FIELD_TMAX 1      // token 9
#define RW_FIELD_TMIN 2      // token 10
#define RW_FIELD_PRCP 3      // token 14
#define RW_NFIELDS 4
#define RW_NTOKENS 15        // an in-period line with fewer raises IndexError

// the token index of a field, and the element plane (GH_ELEM_*) of a value field
GH_HD int rw_field_token(int field) { return field == RW_FIELD_DATE ? 0 : field == RW_FIELD_TMAX ? 9 : field == RW_FIELD_TMIN ? 10 : 14; }
GH_HD int rw_field_elem(int field) { return field == RW_FIELD_TMAX ? GH_ELEM_TMAX : field == RW_FIELD_TMIN ? GH_ELEM_TMIN : GH_ELEM_PRCP; }

// bit k set: byte k of the 16 (little-endian words) is no whitespace and lo <= k < hi
GH_HD uint32_t rw_nonspace16(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, int lo, int hi)
{
    const uint32_t v[4] = {w0, w1, w2, w3};
    uint32_t m = 0;
    for (int k = 0; k < 16; ++k)
        if (k >= lo && k < hi && !gh_space((uint8_t)(v[k >> 2] >> (8 * (k & 3))))) m |= 1u << k;
    return m;
}

// the position of the n-th (0-based) set bit of m; m has more than n bits set
GH_HD int rw_nth_bit(uint32_t m, int n)
{
    for (; n > 0; --n) m &= m - 1;
    int k = 0;
    while (k < 31 && !((m >> k) & 1u)) ++k;
    return k;
}

// the length of the token that starts at s[0], of at most maxn bytes (the line's rest); stops counting at RW_TOK_MAX + 1
GH_HD int rw_token_len(const uint8_t *s, int64_t maxn)
{
    int n = 0;
    while (n < maxn && n <= RW_TOK_MAX && !gh_space(s[n])) ++n;
    return n;
}

// int(s[0 .. n)) of a slice of a token (no whitespace inside): [+-]?[0-9]{1,9}
GH_HD int rw_int(const uint8_t *s, int n, int64_t *v)
{
    int a = 0;
    bool neg = false;
    if (n > 0 && (s[0] == '+' || s[0] == '-')) { neg = s[0] == '-'; a = 1; }
    if (n - a < 1 || n - a > 9) return RW_UNCERTAIN;
    int64_t m = 0;
    for (int i = a; i < n; ++i) {
        if (!gh_digit(s[i])) return RW_UNCERTAIN;
        m = m * 10 + (s[i] - '0');
    }
    *v = neg ? -m : m;
    return RW_OK;
}

// float(s[0 .. n)) of a token: the exact integer of its digits over the exact power of ten, ONE fp64 division: correctly
// rounded, so what float() returns.  "-0" gives -0.0.
GH_HD int rw_float(const uint8_t *s, int n, double *v)
{
    if (n < 1 || n > RW_TOK_MAX) return RW_UNCERTAIN;
    int a = 0;
    bool neg = false;
    if (s[0] == '+' || s[0] == '-') { neg = s[0] == '-'; a = 1; }
    int64_t mant = 0;
    int ndig = 0, nsig = 0, ndec = 0;
    bool point = false;
    for (int i = a; i < n; ++i) {
        const uint8_t c = s[i];
        if (c == '.') {
            if (point) return RW_UNCERTAIN;
            point = true;
        } else if (gh_digit(c)) {
            ++ndig;
            if (point) ++ndec;
            if (nsig > 0 || c != '0') ++nsig;
            if (nsig > 15) return RW_UNCERTAIN;
            mant = mant * 10 + (c - '0');
        } else {
            return RW_UNCERTAIN;
        }
    }
    if (ndig < 1 || ndec > 22) return RW_UNCERTAIN;
    double p = 1.0;                                              // 10^ndec, exact up to 10^22
    for (int i = 0; i < ndec; ++i) p = p * 10.0;
    const double q = (double)mant / p;
    *v = neg ? -q : q;
    return RW_OK;
}

#define RW_DATE_UNCERTAIN 0  // one of the three int() is not the device's to decide
#define RW_DATE_SKIP 1       // no calendar day: the line is skipped and counted
#define RW_DATE_OUTSIDE 2    // a day outside the period: the line is dropped
#define RW_DATE_IN 3         // *day_idx is set

// Token 0 = t[0 .. n): year = int(t[6:]), month = int(t[0:2]), day = int(t[3:5]); bytes 2 and 5 are not looked at.
GH_HD int rw_date(const uint8_t *t, int n, int64_t min_ymd, int64_t max_ymd, int64_t day0, int64_t *day_idx)
{
    if (n > RW_TOK_MAX) return RW_DATE_UNCERTAIN;
    int64_t y = 0, m = 0, d = 0;
    if (rw_int(t + (n < 6 ? n : 6), n < 6 ? 0 : n - 6, &y) != RW_OK) return RW_DATE_UNCERTAIN;
    if (rw_int(t, n < 2 ? n : 2, &m) != RW_OK) return RW_DATE_UNCERTAIN;
    if (rw_int(t + (n < 3 ? n : 3), n < 3 ? 0 : (n < 5 ? n : 5) - 3, &d) != RW_OK) return RW_DATE_UNCERTAIN;
    if (!gh_valid_date(y, m, d)) return RW_DATE_SKIP;
    const int64_t ymd = y * 10000 + m * 100 + d;
    if (ymd < min_ymd || ymd > max_ymd) return RW_DATE_OUTSIDE;
    *day_idx = gh_days_from_civil(y, m, d) - day0;
    return RW_DATE_IN;
}

// A value field's token t[0 .. n) as the float32 of the database: prcp * 0.1 in fp64 unless it is -9999, one rounding.
GH_HD int rw_value(const uint8_t *t, int n, int field, float *out)
{
    double v = 0.0;
    if (rw_float(t, n, &v) != RW_OK) return RW_UNCERTAIN;
    if (field == RW_FIELD_PRCP && v != RW_MISSING) v = v * 0.1;
    *out = (float)v;
    return RW_OK;
}
#endif
