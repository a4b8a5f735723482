/* Stand-in for gr::block: the scheduler-facing surface that the gr-dvbt blocks use, with the
 * behaviour a block's result can depend on and no scheduler:
 *   - one tag list per input with absolute offsets; get_tags_in_range filters it by [start, end) and key
 *   - one output tag list that add_item_tag appends to
 *   - item counters nitems_read / nitems_written, advanced by whoever drives the block
 *   - consume / consume_each record what the block took in the current call
 *   - the tag propagation policy a block asks for is kept for the driver to read
 *   - detail() hands out what the driver set up (gnuradio/block_detail.h): null until it did, as for a block outside a flowgraph
 * The members named si_* are the driver's side (oracle/ref_driver.cc). */
#ifndef REF_STANDIN_GR_BLOCK_H
#define REF_STANDIN_GR_BLOCK_H
#include <gnuradio/types.h>
#include <gnuradio/io_signature.h>
#include <pmt/pmt.h>

namespace gr {

  class block_detail;
  typedef std::shared_ptr<block_detail> block_detail_sptr;

  struct tag_t {
    uint64_t offset;
    pmt::pmt_t key, value, srcid;
    static bool offset_compare(const tag_t &a, const tag_t &b) { return a.offset < b.offset; }
  };

  class block {
  public:
    enum { WORK_CALLED_PRODUCE = -2, WORK_DONE = -1 };
    /* what the scheduler does with the tags of the input items: nothing / every input's to every output / input i's to output i */
    enum tag_propagation_policy_t { TPP_DONT = 0, TPP_ALL_TO_ALL = 1, TPP_ONE_TO_ONE = 2 };

    virtual ~block() {}

    virtual void forecast(int noutput_items, gr_vector_int &ninput_items_required)
    {
      for (size_t i = 0; i < ninput_items_required.size(); i++)
        ninput_items_required[i] = noutput_items;
    }
    virtual int general_work(int, gr_vector_int &, gr_vector_const_void_star &, gr_vector_void_star &) { return WORK_DONE; }

    void consume(int which_input, int how_many_items)
    {
      if ((size_t)which_input >= si_consumed.size()) si_consumed.resize(which_input + 1, 0);
      si_consumed[which_input] += how_many_items;
    }
    void consume_each(int how_many_items)
    {
      for (size_t i = 0; i < si_consumed.size(); i++) si_consumed[i] += how_many_items;
    }

    void set_relative_rate(double r) { si_relative_rate = r; }
    double relative_rate() const { return si_relative_rate; }
    void set_output_multiple(int m) { si_output_multiple = m; }
    int output_multiple() const { return si_output_multiple; }
    void set_alignment(int m) { si_alignment = m; }
    int alignment() const { return si_alignment; }
    void set_tag_propagation_policy(tag_propagation_policy_t p) { si_tpp = p; }
    tag_propagation_policy_t tag_propagation_policy() const { return si_tpp; }
    block_detail_sptr detail() const { return si_detail; }
    virtual bool stop() { return true; }
    bool is_unaligned() const { return false; }   /* the stand-in VOLK kernel is the same either way */

    uint64_t nitems_read(unsigned int which_input) { return which_input < si_nread.size() ? si_nread[which_input] : 0; }
    uint64_t nitems_written(unsigned int which_output) { return which_output < si_nwritten.size() ? si_nwritten[which_output] : 0; }

    void add_item_tag(unsigned int which_output, uint64_t abs_offset, const pmt::pmt_t &key, const pmt::pmt_t &value,
                      const pmt::pmt_t &srcid = pmt::pmt_t())
    {
      si_out_tags.push_back(tag_t{abs_offset, key, value, srcid});
      si_out_tag_port.push_back((int)which_output);
    }
    void add_item_tag(unsigned int which_output, const tag_t &tag) { add_item_tag(which_output, tag.offset, tag.key, tag.value, tag.srcid); }

    void get_tags_in_range(std::vector<tag_t> &v, unsigned int which_input, uint64_t abs_start, uint64_t abs_end)
    {
      v.clear();
      if (which_input >= si_in_tags.size()) return;
      for (const tag_t &t : si_in_tags[which_input])
        if (t.offset >= abs_start && t.offset < abs_end) v.push_back(t);
    }
    void get_tags_in_range(std::vector<tag_t> &v, unsigned int which_input, uint64_t abs_start, uint64_t abs_end, const pmt::pmt_t &key)
    {
      v.clear();
      if (which_input >= si_in_tags.size()) return;
      for (const tag_t &t : si_in_tags[which_input])
        if (t.offset >= abs_start && t.offset < abs_end && pmt::eq(t.key, key)) v.push_back(t);
    }

    const std::string &name() const { return si_name; }
    io_signature::sptr input_signature() const { return si_in_sig; }
    io_signature::sptr output_signature() const { return si_out_sig; }

    /* ---- the driver's side ---- */
    std::string si_name;
    io_signature::sptr si_in_sig, si_out_sig;
    double si_relative_rate = 1.0;
    int si_output_multiple = 1, si_alignment = 1;
    tag_propagation_policy_t si_tpp = TPP_ALL_TO_ALL;   /* GNU Radio's default */
    block_detail_sptr si_detail;
    std::vector<uint64_t> si_nread, si_nwritten;
    std::vector<int> si_consumed;
    std::vector<std::vector<tag_t> > si_in_tags;   /* kept sorted by offset, in the order given within one offset */
    std::vector<tag_t> si_out_tags;
    std::vector<int> si_out_tag_port;

  protected:
    block() {}   /* for the virtual inheritance of the public block classes */
    block(const std::string &name, io_signature::sptr in, io_signature::sptr out)
      : si_name(name), si_in_sig(in), si_out_sig(out),
        si_nread(in->max_streams() > 0 ? in->max_streams() : 1, 0), si_nwritten(out->max_streams() > 0 ? out->max_streams() : 1, 0),
        si_consumed(si_nread.size(), 0), si_in_tags(si_nread.size())
    {
    }
  };

  typedef std::shared_ptr<block> block_sptr;
}

namespace gnuradio {
  template <class T> std::shared_ptr<T> get_initial_sptr(T *p) { return std::shared_ptr<T>(p); }
}
#endif
