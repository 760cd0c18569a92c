/* twx_raws.h -- libtwxqa.so: the RAWS ingest of step04, the library's twentieth unit (topowx_amd/qa/twxrw_raws.hip).  The
 * unit has a header of its own, and topowx_amd/raws.py binds its one entry. */
#ifndef TWX_RAWS_H
#define TWX_RAWS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the RAWS ingest of step04: InsertRaws.parse_stn_obs (twx/db/create_db_all_stations.py:1177-1233) for a batch of WRCC
 * daily listings; topowx_amd/qa/twxrw_raws.hip.  The buffer and the line index are those of twxgh_parse_dly (include/twx_qa.h).  Out of scope: InsertSnotel
 * (its input is made by a module the reference does not hold and parsed by pandas.read_csv), downloading. ---- */
#define TWXRW_NKERNELS 5                /* kernel groups timed: fill; line index; 8th line + "Copyright"; claim pass; write pass */
#define TWXRW_MAX_BYTES ((int64_t)2147483584)   /* of one call's buffer: a line's position + 1 is a uint32 */
#define TWXRW_MAX_CELLS ((int64_t)1 << 31)      /* 3 nfiles ndays */
#define TWXRW_ENTRY_WORDS 8             /* uint32 words of an entry of either list */
#define TWXRW_NO_DAY 0xffffffffu
#define TWXRW_RAISE_EMPTY 0             /* raise list, word 2: a body line without a token (vals[0]: IndexError) */
#define TWXRW_RAISE_FEW 1               /*   an in-period line of fewer than 15 tokens (word 4: how many) */
#define TWXRW_C_LINES 0                 /* counts: lines of the batch */
#define TWXRW_C_BODY 1                  /*   lines from a file's 8th on and before its first line with "Copyright" */
#define TWXRW_C_SKIPPED 2               /*   body lines whose date the device found to be no calendar day */
#define TWXRW_C_VALUES 3                /*   in-period lines whose three values the device decided (duplicates counted each time) */
#define TWXRW_C_DUPLICATES 4            /*   ... of these, the ones a later such line of the same (file, day) overrode */
#define TWXRW_C_UNCERTAIN 5             /*   entries of the uncertain list (may exceed uncertain_cap) */
#define TWXRW_C_RAISE 6                 /*   entries of the raise list (may exceed raise_cap) */
#define TWXRW_C_DATE_UNCERTAIN 7        /*   uncertain entries of field 0; if any, win is filled */
#define TWXRW_C_N 8

/*
 * parse_stn_obs of nfiles listings in one call; file f fills row f of val [3][nfiles][ndays] (TMIN, TMAX, PRCP as in
 * twxgh_parse_dly; float32 pre-set to -9999), ndays the days from min_ymd to max_ymd.
 * Grammar.  A line ends at \n; a last line without one is a line.  The first 7 lines of a file are skipped whatever they
 * hold; of the rest the first line that contains "Copyright" ends the file, itself included.  A token is a maximal run of
 * bytes other than space, \t, \n, \v, \f, \r; there is no cap on a line's length or token count.  With t = token 0: year =
 * int(t[6:]), month = int(t[0:2]), day = int(t[3:5]); no calendar day (years 1 .. 9999): the line is skipped and counted;
 * outside the period: dropped, nothing else of it is looked at.  Else tmax = float(token 9), tmin = float(token 10), prcp =
 * float(token 14) * 0.1 in fp64 unless it is -9999, each rounded once to float32.
 * The device decides an int() field of the form [+-]?[0-9]{1,9} and a float() token of the form [+-]? digits with at most
 * one '.', at least one digit, at most 15 significant digits and at most 22 after the point, as ONE fp64 division of the
 * exact integer by the exact power of ten (correctly rounded, so float()'s value; "-0" is -0.0).  A line with any other
 * field (an exponent, inf / nan, '_', more digits, any other byte, a token of more than 40 bytes) writes nothing and is
 * listed, an entry per such field:
 *   uncertain [uncertain_cap][TWXRW_ENTRY_WORDS] = file, line position in the file, field (0 date, 1 tmax, 2 tmin, 3 prcp),
 *   token offset in the line, token length (41: longer), the position + 1 in the buffer of the decided line that won the
 *   line's (file, day) (0: none, or the day is not known), the day's index (TWXRW_NO_DAY: not known), the line's position
 *   in the buffer; sorted by position, then field.  The caller settles these lines with Python's int() / float().
 *   raise [raise_cap][TWXRW_ENTRY_WORDS]: the lines that raise IndexError or, with a token float() refuses among the first of
 *   a short line, ValueError: same words, word 2 = TWXRW_RAISE_*.
 * Deviation from the reference: when several lines give a day, the LAST decided line wins all three values (the reference
 * fails with ValueError in its chunk assignment): integer atomicMax of the position, no result depends on scheduling or on
 * a capacity, no floating-point atomics.  win [nfiles][ndays]: the winners' positions + 1, written only if
 * counts[TWXRW_C_DATE_UNCERTAIN] > 0.  counts [TWXRW_C_N]; kernel_ms (optional) [TWXRW_NKERNELS].  Every argument is
 * checked before anything touches the device.
 */
int twxrw_parse(int device, const uint8_t *buf, int64_t nbytes, int64_t nfiles, const int64_t *file_off, int32_t min_ymd,
                int32_t max_ymd, int64_t ndays, float *val, uint32_t *win, uint32_t *uncertain, int64_t uncertain_cap,
                uint32_t *raise, int64_t raise_cap, int64_t *counts, float *kernel_ms, char *errbuf, int errlen);

#ifdef __cplusplus
}
#endif
#endif
