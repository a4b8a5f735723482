/* reference_signals_impl.cc -- gr::dvbt::reference_signals on libdvbt_hip (replaces lib/reference_signals_impl.cc).  symbol_index and frame_index are carried in the handle, from 0. */
#include "reference_signals_impl.h"

namespace gr {
  namespace dvbt {

    reference_signals::sptr
    reference_signals::make(int itemsize, int ninput, int noutput, dvbt_constellation_t constellation, dvbt_hierarchy_t hierarchy, dvbt_code_rate_t code_rate_HP, dvbt_code_rate_t code_rate_LP, dvbt_guard_interval_t guard_interval, dvbt_transmission_mode_t transmission_mode, int include_cell_id, int cell_id)
    { return gnuradio::get_initial_sptr(new reference_signals_impl(itemsize, ninput, noutput, constellation, hierarchy, code_rate_HP, code_rate_LP, guard_interval, transmission_mode, include_cell_id, cell_id)); }

    static dvbt_reference_signals_params reference_signals_params(int itemsize, int ninput, int noutput, int constellation, int hierarchy, int code_rate_HP, int code_rate_LP, int guard_interval, int transmission_mode, int include_cell_id, int cell_id)
    { dvbt_reference_signals_params q = { itemsize, ninput, noutput, constellation, hierarchy, code_rate_HP, code_rate_LP, guard_interval, transmission_mode, include_cell_id, cell_id }; return q; }

    /* io signatures and scheduler hints: lib/reference_signals_impl.cc:1254-1266 */
    reference_signals_impl::reference_signals_impl(int itemsize, int ninput, int noutput, dvbt_constellation_t constellation, dvbt_hierarchy_t hierarchy, dvbt_code_rate_t code_rate_HP, dvbt_code_rate_t code_rate_LP, dvbt_guard_interval_t guard_interval, dvbt_transmission_mode_t transmission_mode, int include_cell_id, int cell_id)
      : block("reference_signals", io_signature::make(1, 1, itemsize * ninput), io_signature::make(1, 1, itemsize * noutput)),
        DVBT_HIP_CORE_INIT(reference_signals, reference_signals_params(itemsize, ninput, noutput, constellation, hierarchy, code_rate_HP, code_rate_LP, guard_interval, transmission_mode, include_cell_id, cell_id))
    {
    }

  } /* namespace dvbt */
} /* namespace gr */
