"""``TimeAxis.year_month`` and ``date_from_days`` (ace_amd/timeaxis.py): the inverse of ``days_since_base`` for the six calendars,
across leap days and across the 1582 switch of ``standard``."""
import datetime

import numpy as np
import pytest

from ace_amd.timeaxis import CALENDARS, TimeAxis, date_from_days, days_since_base

DATES = [(1, 1, 1), (1, 12, 31), (4, 2, 28), (4, 3, 1), (100, 2, 28), (100, 3, 1), (400, 12, 31), (1582, 10, 4), (1582, 10, 15),
         (1582, 12, 31), (1583, 1, 1), (1600, 2, 28), (1600, 3, 1), (1700, 2, 28), (1700, 3, 1), (1900, 2, 28), (1900, 3, 1),
         (1999, 12, 31), (2000, 1, 1), (2000, 2, 28), (2000, 3, 1), (2001, 1, 31), (2001, 2, 1), (2024, 2, 28), (2024, 12, 30),
         (2100, 3, 1), (9999, 12, 30)]


@pytest.mark.parametrize("calendar", CALENDARS)
def test_year_month_round_trips_from_components(calendar):
    comps = np.array([d + (h, 30, 0) for d in DATES for h in (0, 23)])
    if calendar == "360_day":
        comps[:, 2] = np.minimum(comps[:, 2], 30)
    axis = TimeAxis.from_components(calendar, comps.reshape(2, -1, 6))
    year, month = axis.year_month()
    assert year.shape == month.shape == axis.shape and year.dtype == month.dtype == np.int64
    assert np.array_equal(year, comps[:, 0].reshape(2, -1)) and np.array_equal(month, comps[:, 1].reshape(2, -1))
    y, m, d = date_from_days(calendar, axis.us // 86_400_000_000)
    assert np.array_equal(d, comps[:, 2].reshape(2, -1))


@pytest.mark.parametrize("calendar", CALENDARS)
def test_every_day_of_five_centuries_inverts(calendar):
    """1400-01-01 .. 1900: through Julian and Gregorian century years and, for ``standard``, the ten days that do not exist"""
    first, last = (int(days_since_base(calendar, y, 1, 1)) for y in (1400, 1900))
    days = np.arange(first, last)
    y, m, d = date_from_days(calendar, days)
    assert np.array_equal(days_since_base(calendar, y, m, d), days)
    assert np.all(np.diff(y * 10000 + m * 100 + d) > 0)                                  # strictly increasing dates


def test_leap_days():
    for calendar, year, leap in (("standard", 1500, True), ("proleptic_gregorian", 1500, False), ("julian", 1900, True),
                                 ("standard", 1900, False), ("standard", 2000, True), ("noleap", 2000, False), ("all_leap", 2001, True)):
        day59 = date_from_days(calendar, days_since_base(calendar, year, 1, 1) + 59)       # the 60th day of the year
        assert tuple(int(v) for v in day59) == ((year, 2, 29) if leap else (year, 3, 1)), (calendar, year)
    assert tuple(int(v) for v in date_from_days("360_day", days_since_base("360_day", 2000, 1, 1) + 59)) == (2000, 2, 30)


def test_the_1582_switch_of_the_standard_calendar():
    start = days_since_base("standard", 1582, 10, 1)
    y, m, d = date_from_days("standard", start + np.arange(8))
    assert m.tolist() == [10] * 8 and d.tolist() == [1, 2, 3, 4, 15, 16, 17, 18] and set(y.tolist()) == {1582}
    assert int(days_since_base("standard", 1583, 1, 1) - days_since_base("standard", 1582, 1, 1)) == 355
    step = TimeAxis.regular((1582, 9, 20), datetime.timedelta(days=5), 6, n_samples=1, calendar="standard")
    assert step.year_month()[1].tolist() == [[9, 9, 9, 10, 10, 10]]                     # ... 09-30, 10-15 (5 days on), 10-20, 10-25
    proleptic = date_from_days("proleptic_gregorian", days_since_base("proleptic_gregorian", 1582, 10, 4) + 1)
    assert tuple(int(v) for v in proleptic) == (1582, 10, 5)


def test_years_before_one_are_refused():
    with pytest.raises(ValueError, match="before 1"):
        date_from_days("noleap", [-1])
