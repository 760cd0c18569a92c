// twx_ghcn_field.h -- the field logic of the GHCN-Daily ingest (twx_ghcn.hip): calendar, clipping, the grammar of a number
// and the unit conversion, as __host__ __device__ functions of bytes already in hand.  The kernels call them on lines staged
// in LDS; tests/tools/ghcn_hostcheck.cpp calls the same code on the CPU (g++, address and undefined-behaviour sanitizers).
// Nothing here touches memory outside [s, s + n): every caller clips n to the line's own end first.
//
// Reference: InsertGhcn.parse_stn_obs / __convert_units (twx/db/create_db_all_stations.py:1028-1103) and create_tobs_db
// (twx/homog/tobs.py:121-157).  "Whitespace" is what bytes.strip(), int() and float() strip: space, \t, \n, \v, \f, \r.
#ifndef TWX_GHCN_FIELD_H
#define TWX_GHCN_FIELD_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GH_HD __host__ __device__ __forceinline__
#else
#define GH_HD inline
#endif

#define GH_NUM_OK 0          // [+-]?[0-9]+ after the strip
#define GH_NUM_EMPTY 1       // nothing but whitespace (or no bytes at all): int() / float() raise ValueError
#define GH_NUM_OTHER 2       // any other text: Python decides it (' 1.5e', 'nan', '1e3', '1_0', ...)

#define GH_ELEM_TMIN 0
#define GH_ELEM_TMAX 1
#define GH_ELEM_PRCP 2
#define GH_ELEM_NONE (-1)

#define GH_LINE_BYTES 272    // no byte past 21 + 8 * 30 + 7 = 268 of a .dly line is ever read
#define GH_MISSING (-9999.0)

GH_HD bool gh_space(uint8_t c) { return c == 0x20 || (c >= 0x09 && c <= 0x0d); }
GH_HD bool gh_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// The number in s[0 .. n) (n <= 0: empty).  On GH_NUM_OK *mag is the magnitude (saturating far above anything a field of
// these widths holds) and *neg its sign: "-0" keeps the sign, as float("-0") does.
GH_HD int gh_number(const uint8_t *s, int n, int64_t *mag, bool *neg)
{
    int a = 0, b = n;
    while (a < b && gh_space(s[a])) ++a;
    while (b > a && gh_space(s[b - 1])) --b;
    if (a >= b) return GH_NUM_EMPTY;
    bool ng = false;
    if (s[a] == '+' || s[a] == '-') { ng = s[a] == '-'; ++a; }
    if (a >= b) return GH_NUM_OTHER;
    int64_t v = 0;
    for (int i = a; i < b; ++i) {
        if (!gh_digit(s[i])) return GH_NUM_OTHER;
        if (v < ((int64_t)1 << 56)) v = v * 10 + (s[i] - '0');
    }
    *mag = v;
    *neg = ng;
    return GH_NUM_OK;
}

GH_HD bool gh_leap(int64_t y) { return (y % 4 == 0 && y % 100 != 0) || y % 400 == 0; }

// datetime.date(y, m, d) would not raise: proleptic Gregorian, years 1 .. 9999
GH_HD bool gh_valid_date(int64_t y, int64_t m, int64_t d)
{
    if (y < 1 || y > 9999 || m < 1 || m > 12 || d < 1) return false;
    const int dim = (m == 2) ? (gh_leap(y) ? 29 : 28) : ((m == 4 || m == 6 || m == 9 || m == 11) ? 30 : 31);
    return d <= dim;
}

// days since 1970-01-01 of a valid date (integer arithmetic; era = 400 years)
GH_HD int64_t gh_days_from_civil(int64_t y, int64_t m, int64_t d)
{
    y -= m <= 2;
    const int64_t era = (y >= 0 ? y : y - 399) / 400;
    const int64_t yoe = y - era * 400;
    const int64_t doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
    const int64_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
    return era * 146097 + doe - 719468;
}

// line[17:21].strip() in ("TMIN", "TMAX", "PRCP"): four bytes, so the strip can only shorten it out of the list
GH_HD int gh_element(const uint8_t *line, int len)
{
    if (len < 21) return GH_ELEM_NONE;
    const uint8_t *e = line + 17;
    if (e[0] == 'T' && e[1] == 'M' && e[2] == 'I' && e[3] == 'N') return GH_ELEM_TMIN;
    if (e[0] == 'T' && e[1] == 'M' && e[2] == 'A' && e[3] == 'X') return GH_ELEM_TMAX;
    if (e[0] == 'P' && e[1] == 'R' && e[2] == 'C' && e[3] == 'P') return GH_ELEM_PRCP;
    return GH_ELEM_NONE;
}

// int(line[11:15]) and int(line[15:17]) of a line of len bytes: GH_NUM_OK only if both are canonical
GH_HD int gh_header(const uint8_t *line, int len, int64_t *year, int64_t *month)
{
    int64_t mag = 0;
    bool neg = false;
    int hi = len < 15 ? len : 15;
    int rc = gh_number(line + (len < 11 ? len : 11), hi - 11, &mag, &neg);
    if (rc != GH_NUM_OK) return rc;
    *year = neg ? -mag : mag;
    hi = len < 17 ? len : 17;
    rc = gh_number(line + (len < 15 ? len : 15), hi - 15, &mag, &neg);
    if (rc != GH_NUM_OK) return rc;
    *month = neg ? -mag : mag;
    return GH_NUM_OK;
}

// __convert_units on the float64 of the field, then the assignment into the float32 chunk: one rounding
GH_HD float gh_convert(int elem, int64_t mag, bool neg)
{
    const double v = neg ? -(double)mag : (double)mag;
    if (v == GH_MISSING) return (float)v;
    return (float)(elem == GH_ELEM_PRCP ? v / 100.0 : v / 10.0);
}

#define GH_FIELD_SKIP 0      // invalid date, outside the period, or an empty value: nothing is written
#define GH_FIELD_VALUE 1     // *value, *qflag and *day_idx are set
#define GH_FIELD_PYTHON 2    // in the period, text only float() can decide: *day_idx is set

// Day field d (0 .. 30) of a line whose header gave (year, month, elem).  day0 = gh_days_from_civil of min_ymd.
GH_HD int gh_field(const uint8_t *line, int len, int64_t year, int64_t month, int elem, int d, int64_t min_ymd,
                   int64_t max_ymd, int64_t day0, float *value, uint8_t *qflag, int64_t *day_idx)
{
    const int64_t day = d + 1;
    if (!gh_valid_date(year, month, day)) return GH_FIELD_SKIP;
    const int64_t ymd = year * 10000 + month * 100 + day;
    if (ymd < min_ymd || ymd > max_ymd) return GH_FIELD_SKIP;
    const int s = 21 + 8 * d;
    const int e = len < s + 5 ? len : s + 5;
    int64_t mag = 0;
    bool neg = false;
    const int rc = gh_number(line + (len < s ? len : s), e - s, &mag, &neg);
    if (rc == GH_NUM_EMPTY) return GH_FIELD_SKIP;
    *day_idx = gh_days_from_civil(year, month, day) - day0;
    if (rc == GH_NUM_OTHER) return GH_FIELD_PYTHON;
    *value = gh_convert(elem, mag, neg);
    uint8_t q = (s + 6 < len) ? line[s + 6] : 0;
    if (gh_space(q)) q = 0;
    *qflag = q;
    return GH_FIELD_VALUE;
}

// ---- the by-year CSV line: ID(11),YYYYMMDD(8),ELEM(4),value,m,q,s,HHMM ----
#define GH_TOBS_SKIP 0       // not selected by the filter, or a date that is no day of the period
#define GH_TOBS_VALUE 1
#define GH_TOBS_BAD 2        // selected, known station: int(line[-5:]) or int(line[12:20]) is not canonical
#define GH_TOBS_OUTSIDE 3    // selected, known station, a date outside the period (counted)

// The filter of create_tobs_file (tobs.py:61-62) restated on one line WITHOUT its newline (grep's view): the element field
// line[21:25] equals elem4, the id starts with US / CA / MX, the last character is a digit, the line does not end in 2400.
GH_HD bool gh_tobs_selected(const uint8_t *line, int len, const uint8_t *elem4)
{
    if (len < 25) return false;
    for (int i = 0; i < 4; ++i)
        if (line[21 + i] != elem4[i]) return false;
    const bool fips = (line[0] == 'U' && line[1] == 'S') || (line[0] == 'C' && line[1] == 'A') ||
                      (line[0] == 'M' && line[1] == 'X');
    if (!fips || !gh_digit(line[len - 1])) return false;
    if (line[len - 4] == '2' && line[len - 3] == '4' && line[len - 2] == '0' && line[len - 1] == '0') return false;
    return true;
}

// What create_tobs_db (tobs.py:146-151) does with a selected line of a known station, in its order: int(line[12:20]), the
// day's index, int(line[-5:]) of the line WITH its newline: the last four characters.  Every line of the tobs file has one,
// the last line of a by-year file too: grep ends each line it prints with a newline.  len >= 25 (gh_tobs_selected).  A
// value that does not fit int16 is GH_TOBS_BAD.
GH_HD int gh_tobs_fields(const uint8_t *line, int len, int64_t min_ymd, int64_t max_ymd, int64_t day0,
                         int64_t *day_idx, int32_t *value)
{
    int64_t mag = 0;
    bool neg = false;
    if (gh_number(line + 12, 8, &mag, &neg) != GH_NUM_OK) return GH_TOBS_BAD;
    const int64_t ymd = neg ? -mag : mag;
    if (ymd < min_ymd || ymd > max_ymd) return GH_TOBS_OUTSIDE;
    const int64_t y = ymd / 10000, m = (ymd / 100) % 100, d = ymd % 100;
    if (!gh_valid_date(y, m, d)) return GH_TOBS_OUTSIDE;
    const int n = 4;
    if (gh_number(line + len - n, n, &mag, &neg) != GH_NUM_OK || mag > 32767) return GH_TOBS_BAD;
    *day_idx = gh_days_from_civil(y, m, d) - day0;
    *value = (int32_t)(neg ? -mag : mag);
    return GH_TOBS_VALUE;
}
#endif
