// qhip_datetime.inc — the date code of EXTRACT(part FROM date / timestamp) (physical/expr/function.rs ->
// functions/datetime/extract.rs -> arrow-rs 53 `date_part`, cast to Int64).
//
// One text for three compilers: pasted into the hiprtc string by embed.py (generated policies call it per row), included by
// qhip_device.hpp for hipcc, and included as plain host C++ by expr.cpp (literal folding) and tests/cpp/datetime_parts.cpp
// (checked against pyarrow). Self-contained: builtin integer types only, no #include.
//
// gfx950 has no integer divide instruction, so every division below is by a constant (the compiler turns it into a
// multiply-high sequence) and, after the timestamp split, in 32-bit unsigned arithmetic: offsets make every dividend
// non-negative. Only qh_dt_split touches 64-bit values.
#if defined(__HIP__) || defined(__HIPCC_RTC__)
#define QH_HD __host__ __device__
#else
#define QH_HD
#endif

// part ids: the order of the structural suffix in the canonical form `extract[<part>](...)` (expr.cpp)
#define QH_DT_YEAR 0
#define QH_DT_MONTH 1
#define QH_DT_DAY 2
#define QH_DT_HOUR 3
#define QH_DT_MINUTE 4
#define QH_DT_SECOND 5
#define QH_DT_WEEK 6

// Days since 1970-01-01 that chrono's NaiveDate can represent (-262144-01-01 ... +262143-12-31). arrow's as_datetime returns
// None outside, and its unary_opt makes that row NULL. THE place that decides the range.
#define QH_DT_MIN_DAYS (-96465658)
#define QH_DT_MAX_DAYS 95026601
QH_HD inline bool qh_dt_in_range(long long days) { return days >= QH_DT_MIN_DAYS && days <= QH_DT_MAX_DAYS; }

// Date32 has no time of day: arrow-rs's Date32 kernel returns zeros (with the input's validity, no range check) for the time
// parts. THE place that decides it: true = the part of a Date32 is the constant 0.
QH_HD inline bool qh_dt_date32_zero_part(int part) { return part == QH_DT_HOUR || part == QH_DT_MINUTE || part == QH_DT_SECOND; }

struct qh_civil {
  int year, month, day;
  int yday;    // 0-based day of the civil year (Jan 1 = 0)
  int leap0;   // 1 when the March-based year of the date (Mar 1 .. end of Feb) starts in a leap civil year
};

// civil-from-days (H. Hinnant's algorithm), 32-bit unsigned: the offset (a whole number of 400-year eras, 146097 days each)
// makes every in-range day count positive; out-of-range values wrap harmlessly (their rows are NULL anyway)
#define QH_DT_ERAS 700u
QH_HD inline qh_civil qh_dt_civil(int days) {
  const unsigned z = (unsigned)days + 719468u + QH_DT_ERAS * 146097u;
  const unsigned era = z / 146097u;
  const unsigned doe = z - era * 146097u;                                          // [0, 146096]
  const unsigned yoe = (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u;  // [0, 399]
  const unsigned doy = doe - (365u * yoe + yoe / 4u - yoe / 100u);                 // [0, 365], 0 = March 1
  const unsigned mp = (5u * doy + 2u) / 153u;                                      // [0, 11], 0 = March
  qh_civil c;
  c.day = (int)(doy - (153u * mp + 2u) / 5u + 1u);
  c.month = (int)(mp < 10u ? mp + 3u : mp - 9u);
  c.leap0 = ((yoe & 3u) == 0u && yoe % 100u != 0u) || yoe == 0u;
  c.year = (int)(yoe + era * 400u) - (int)(QH_DT_ERAS * 400u) + (mp >= 10u ? 1 : 0);
  c.yday = mp >= 10u ? (int)doy - 306 : (int)doy + 59 + c.leap0;
  return c;
}

// ISO-8601 week (chrono's iso_week().week()): the week of the Thursday of the date's Monday-based week, counted from the
// first Thursday of that Thursday's year
QH_HD inline int qh_dt_iso_week(int days, const qh_civil& c) {
  const int wd = (int)(((unsigned)days + 98000003u) % 7u);   // 0 = Monday (1970-01-01 was a Thursday: 98000003 = 7 * 14000000 + 3)
  int t = c.yday - wd + 3;                                     // day of the civil year of that Thursday
  const int len = 365 + c.leap0;                               // (only a January date can fall back, only a December one forward:
  if (t < 0) t += len;                                         //  both years' lengths are the March-based year's)
  else if (t >= len) t -= len;
  return t / 7 + 1;
}

// time-of-day parts from the second of the day [0, 86399]
QH_HD inline int qh_dt_time_part(int part, int sod) {
  const unsigned s = (unsigned)sod;
  return part == QH_DT_HOUR ? (int)(s / 3600u) : part == QH_DT_MINUTE ? (int)(s / 60u % 60u) : (int)(s % 60u);
}

// value of `part` for a day count (and second of the day); the part is a compile-time constant in the generated code
QH_HD inline int qh_dt_part(int part, int days, int sod) {
  if (part == QH_DT_HOUR || part == QH_DT_MINUTE || part == QH_DT_SECOND) return qh_dt_time_part(part, sod);
  const qh_civil c = qh_dt_civil(days);
  return part == QH_DT_YEAR ? c.year : part == QH_DT_MONTH ? c.month : part == QH_DT_DAY ? c.day : qh_dt_iso_week(days, c);
}

// Timestamp / Date64 split: ONE floor division of the i64 by the constant 86400 * units-per-second gives the day count and
// the second of the day (arrow's as_datetime floors too: -1 ms is 1969-12-31 23:59:59). UNITS_LOG10: 0 s, 3 ms, 6 us, 9 ns.
// Returns whether the day is inside chrono's range; days / sod are only meaningful then.
template <int UNITS_LOG10> QH_HD inline bool qh_dt_split(long long v, int& days, int& sod) {
  const long long per_sec = UNITS_LOG10 == 0 ? 1LL : UNITS_LOG10 == 3 ? 1000LL : UNITS_LOG10 == 6 ? 1000000LL : 1000000000LL;
  const long long per_day = 86400LL * per_sec;
  long long q = v / per_day;
  long long r = v - q * per_day;
  if (r < 0) { q -= 1; r += per_day; }
  days = (int)q;
  // r < 86400 * per_sec: 32 bits for s / ms; us: r / 2^6 < 2^31 before the division by 15625; ns stays 64-bit
  if (UNITS_LOG10 == 0) sod = (int)r;
  else if (UNITS_LOG10 == 3) sod = (int)((unsigned)r / 1000u);
  else if (UNITS_LOG10 == 6) sod = (int)((unsigned)((unsigned long long)r >> 6) / 15625u);
  else sod = (int)((unsigned long long)r / 1000000000ULL);
  return qh_dt_in_range(q);
}

// EXTRACT(part FROM v) for one value. UNIT: -1 = Date32 (days), 0 / 3 / 6 / 9 = Timestamp(s / ms / us / ns); Date64 is 3.
// Returns false for a NULL result (outside chrono's range); `out` is then meaningless. The generated code passes PART and
// UNIT as constants, so everything but one path folds away.
QH_HD inline bool qh_dt_extract(int part, int unit, long long v, long long& out) {
  int days = 0, sod = 0;
  bool ok;
  if (unit < 0) {
    if (qh_dt_date32_zero_part(part)) { out = 0; return true; }
    days = (int)v;
    ok = qh_dt_in_range(days);
  } else {
    ok = unit == 0 ? qh_dt_split<0>(v, days, sod) : unit == 3 ? qh_dt_split<3>(v, days, sod)
       : unit == 6 ? qh_dt_split<6>(v, days, sod) : qh_dt_split<9>(v, days, sod);
  }
  out = (long long)qh_dt_part(part, days, sod);
  return ok;
}
