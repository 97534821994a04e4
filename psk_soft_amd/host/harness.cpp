// harness.cpp -- in-memory ports + a C API so that Python tests can drive the C++ host class
// (psk_soft_gpu.h) the way the reference's test drives the sandbox-launched component
// (reference tests/test_psk_soft.py:119-269): configure properties, push a packet into the
// input port, run serviceFunction(), read what the four output ports received.
// Test support only; not part of libpsk_soft_hip.so.
#include <deque>
#include <string>
#include <vector>

#include "psk_soft_gpu.h"

namespace {

struct StreamSRI {
    double xdelta;
    int mode;
    std::string streamID;
};
struct Time {
    double twsec, tfsec;
};

// dataFloat_in (T = float), dataShort_in (T = short: complex int16 packets) or dataChar_in (T = char: complex int8 packets)
// (live: the dataTransfer objects of this port that exist, queued or handed out by getPacket and not yet deleted -- the component
// owns what it takes, and psk_harness_live_packets shows a packet it forgot)
template <class Sample>
struct InPort {
    struct dataTransfer {
        std::vector<Sample> dataBuffer;
        StreamSRI SRI;
        Time T;
        bool EOS;
        std::string streamID;
        bool sriChanged;
        bool inputQueueFlushed;
        explicit dataTransfer(int *live_) : live(live_) { ++*live; }
        ~dataTransfer() { --*live; }

      private:
        int *live;
        dataTransfer(const dataTransfer &);
        dataTransfer &operator=(const dataTransfer &);
    };
    std::deque<dataTransfer *> q;
    int live;
    InPort() : live(0) {}
    dataTransfer *getPacket(float)
    {
        if (q.empty())
            return 0;
        dataTransfer *p = q.front();
        q.pop_front();
        return p;
    }
    ~InPort()
    {
        for (size_t i = 0; i < q.size(); i++) delete q[i];
    }
};

template <class T>
struct OutPort {
    std::vector<T> data;           // payload of every pushPacket since the last drain
    std::vector<double> sri_xdelta;  // xdelta of every pushSRI
    std::vector<int> sri_mode;
    int n_packets;
    bool last_eos;
    std::string last_stream;
    double last_twsec;
    OutPort() : n_packets(0), last_eos(false), last_twsec(0) {}
    void pushSRI(const StreamSRI &s)
    {
        sri_xdelta.push_back(s.xdelta);
        sri_mode.push_back(s.mode);
    }
    void pushPacket(std::vector<T> &v, const Time &t, bool eos, const std::string &id)
    {
        data.insert(data.end(), v.begin(), v.end());
        n_packets++;
        last_eos = eos;
        last_stream = id;
        last_twsec = t.twsec;
    }
};

typedef psk_soft_gpu::component<InPort<float>, OutPort<float>, OutPort<short> > Component;
typedef psk_soft_gpu::component<InPort<short>, OutPort<float>, OutPort<short> > ShortComponent;
// (plain char, as some BULKIO releases type dataChar buffers: psk_soft_gpu.h reads it as int8_t)
typedef psk_soft_gpu::component<InPort<char>, OutPort<float>, OutPort<short> > CharComponent;

// one of the three components: float input (psk_harness_create), short input (psk_harness_create_i16) or char input
// (psk_harness_create_i8)
struct Harness {
    InPort<float> in;
    InPort<short> in_s;
    InPort<char> in_c;
    OutPort<float> soft, phase;
    OutPort<short> bits, sidx;
    Component *comp;
    ShortComponent *comp_s;
    CharComponent *comp_c;
    std::string error;
    template <class C>
    void wire(C &c)
    {
        c.softDecision_dataFloat_out = &soft;
        c.bits_dataShort_out = &bits;
        c.phase_dataFloat_out = &phase;
        c.sampleIndex_dataShort_out = &sidx;
    }
    // input: 0 float, 1 short, 2 char
    Harness(int device, int input) : comp(0), comp_s(0), comp_c(0)
    {
        if (input == 1) {
            comp_s = new ShortComponent(device);
            comp_s->dataFloat_in = &in_s;
            wire(*comp_s);
        } else if (input == 2) {
            comp_c = new CharComponent(device);
            comp_c->dataFloat_in = &in_c;
            wire(*comp_c);
        } else {
            comp = new Component(device);
            comp->dataFloat_in = &in;
            wire(*comp);
        }
    }
    ~Harness()
    {
        delete comp;
        delete comp_s;
        delete comp_c;
    }
};

template <class C>
void configure_prop(C &c, int id, unsigned value)
{
    switch (id) {
    case 0: { bool ch = c.samplesPerBaud != value; c.samplesPerBaud = (unsigned short)value; if (ch) c.samplesPerBaudChanged("samplesPerBaud"); break; }
    case 1: c.numAvg = value; break;
    case 2: { bool ch = c.constelationSize != value; c.constelationSize = (unsigned short)value; if (ch) c.constelationSizeChanged("constelationSize"); break; }
    case 3: { bool ch = c.phaseAvg != value; c.phaseAvg = (unsigned short)value; if (ch) c.phaseAvgChanged("phaseAvg"); break; }
    case 4: c.differentialDecoding = value != 0; break;
    case 5: c.resetState = value != 0; break;
    }
}

template <class T>
void push_packet(InPort<T> &in, const T *data, size_t n, double xdelta, int mode, int sriChanged, int flushed, int eos,
                 const char *streamID, double twsec)
{
    typename InPort<T>::dataTransfer *p = new typename InPort<T>::dataTransfer(&in.live);
    p->dataBuffer.assign(data, data + n);
    p->SRI.xdelta = xdelta;
    p->SRI.mode = mode;
    p->SRI.streamID = streamID ? streamID : "";
    p->T.twsec = twsec;
    p->T.tfsec = 0;
    p->EOS = eos != 0;
    p->streamID = p->SRI.streamID;
    p->sriChanged = sriChanged != 0;
    p->inputQueueFlushed = flushed != 0;
    in.q.push_back(p);
}

template <class C>
long get_prop(const C &c, int id)
{
    switch (id) {
    case 0: return c.samplesPerBaud;
    case 1: return (long)c.numAvg;
    case 2: return c.constelationSize;
    case 3: return c.phaseAvg;
    case 4: return c.differentialDecoding ? 1 : 0;
    case 5: return c.resetState ? 1 : 0;
    }
    return -1;
}

}  // namespace

extern "C" {

static void *create(int device, int input, char *err, int errlen)
{
    try {
        return new Harness(device, input);
    } catch (const std::exception &e) {
        if (err && errlen > 0) {
            std::string m = e.what();
            size_t n = m.size() < (size_t)errlen - 1 ? m.size() : (size_t)errlen - 1;
            for (size_t i = 0; i < n; i++) err[i] = m[i];
            err[n] = 0;
        }
        return 0;
    }
}
void *psk_harness_create(int device, char *err, int errlen) { return create(device, 0, err, errlen); }
// a component whose input is a short port (complex int16 packets, PSK_SOFT_FORMAT_CS16)
void *psk_harness_create_i16(int device, char *err, int errlen) { return create(device, 1, err, errlen); }
// a component whose input is a char port (complex int8 packets, PSK_SOFT_FORMAT_CS8)
void *psk_harness_create_i8(int device, char *err, int errlen) { return create(device, 2, err, errlen); }
void psk_harness_destroy(void *h) { delete (Harness *)h; }

// configure() of one property: stores it and, like REDHAWK's PropertySet, runs the registered
// change listener when the value changed.  id: 0 samplesPerBaud 1 numAvg 2 constelationSize
// 3 phaseAvg 4 differentialDecoding 5 resetState
int psk_harness_configure(void *hv, int id, unsigned value)
{
    Harness *h = (Harness *)hv;
    if (id < 0 || id > 5)
        return -1;
    try {
        if (h->comp)
            configure_prop(*h->comp, id, value);
        else if (h->comp_s)
            configure_prop(*h->comp_s, id, value);
        else
            configure_prop(*h->comp_c, id, value);
    } catch (const std::exception &e) {
        h->error = e.what();
        return -2;
    }
    return 0;
}

void psk_harness_push(void *hv, const float *data, size_t n_floats, double xdelta, int mode, int sriChanged,
                      int flushed, int eos, const char *streamID, double twsec)
{
    push_packet(((Harness *)hv)->in, data, n_floats, xdelta, mode, sriChanged, flushed, eos, streamID, twsec);
}
// (short-input component) n_shorts int16 elements, interleaved I,Q
void psk_harness_push_i16(void *hv, const short *data, size_t n_shorts, double xdelta, int mode, int sriChanged,
                          int flushed, int eos, const char *streamID, double twsec)
{
    push_packet(((Harness *)hv)->in_s, data, n_shorts, xdelta, mode, sriChanged, flushed, eos, streamID, twsec);
}
// (char-input component) n_chars int8 elements, interleaved I,Q
void psk_harness_push_i8(void *hv, const signed char *data, size_t n_chars, double xdelta, int mode, int sriChanged,
                         int flushed, int eos, const char *streamID, double twsec)
{
    push_packet(((Harness *)hv)->in_c, reinterpret_cast<const char *>(data), n_chars, xdelta, mode, sriChanged, flushed, eos, streamID,
                twsec);
}

int psk_harness_service(void *hv)
{
    Harness *h = (Harness *)hv;
    try {
        return h->comp ? h->comp->serviceFunction() : h->comp_s ? h->comp_s->serviceFunction() : h->comp_c->serviceFunction();
    } catch (const std::exception &e) {
        h->error = e.what();
        return -1;
    }
}
const char *psk_harness_error(void *hv) { return ((Harness *)hv)->error.c_str(); }
int psk_harness_warnings(void *hv)
{
    Harness *h = (Harness *)hv;
    return h->comp ? h->comp->warnings : h->comp_s ? h->comp_s->warnings : h->comp_c->warnings;
}

// port: 0 soft 1 bits 2 phase 3 sampleIndex
static size_t port_size(Harness *h, int port)
{
    switch (port) {
    case 0: return h->soft.data.size();
    case 1: return h->bits.data.size();
    case 2: return h->phase.data.size();
    default: return h->sidx.data.size();
    }
}
size_t psk_harness_port_size(void *hv, int port) { return port_size((Harness *)hv, port); }
int psk_harness_port_packets(void *hv, int port)
{
    Harness *h = (Harness *)hv;
    switch (port) {
    case 0: return h->soft.n_packets;
    case 1: return h->bits.n_packets;
    case 2: return h->phase.n_packets;
    default: return h->sidx.n_packets;
    }
}
// copies and drains the accumulated payload of one port (getData() of a sandbox DataSink)
size_t psk_harness_port_read_f32(void *hv, int port, float *dst, size_t cap)
{
    Harness *h = (Harness *)hv;
    std::vector<float> &v = port == 0 ? h->soft.data : h->phase.data;
    size_t n = v.size() < cap ? v.size() : cap;
    for (size_t i = 0; i < n; i++) dst[i] = v[i];
    v.clear();
    return n;
}
size_t psk_harness_port_read_i16(void *hv, int port, short *dst, size_t cap)
{
    Harness *h = (Harness *)hv;
    std::vector<short> &v = port == 1 ? h->bits.data : h->sidx.data;
    size_t n = v.size() < cap ? v.size() : cap;
    for (size_t i = 0; i < n; i++) dst[i] = v[i];
    v.clear();
    return n;
}
// pushSRI log of one port: returns count, fills xdelta / mode of the most recent `cap` entries
size_t psk_harness_port_sri(void *hv, int port, double *xdelta, int *mode, size_t cap)
{
    Harness *h = (Harness *)hv;
    std::vector<double> *x;
    std::vector<int> *m;
    switch (port) {
    case 0: x = &h->soft.sri_xdelta; m = &h->soft.sri_mode; break;
    case 1: x = &h->bits.sri_xdelta; m = &h->bits.sri_mode; break;
    case 2: x = &h->phase.sri_xdelta; m = &h->phase.sri_mode; break;
    default: x = &h->sidx.sri_xdelta; m = &h->sidx.sri_mode; break;
    }
    size_t n = x->size();
    for (size_t i = 0; i < n && i < cap; i++) {
        xdelta[i] = (*x)[i];
        mode[i] = (*m)[i];
    }
    return n;
}
int psk_harness_last_eos(void *hv) { return ((Harness *)hv)->soft.last_eos ? 1 : 0; }
const char *psk_harness_last_stream(void *hv) { return ((Harness *)hv)->soft.last_stream.c_str(); }
// dataTransfer objects of the input port that exist: the queued ones, and any that a serviceFunction() took and did not delete
int psk_harness_live_packets(void *hv)
{
    Harness *h = (Harness *)hv;
    return h->in.live + h->in_s.live + h->in_c.live;
}
// a property as the component holds it now (resetState: as the last serviceFunction() left it).  ids as psk_harness_configure
long psk_harness_property(void *hv, int id)
{
    Harness *h = (Harness *)hv;
    return h->comp ? get_prop(*h->comp, id) : h->comp_s ? get_prop(*h->comp_s, id) : get_prop(*h->comp_c, id);
}
// the component's library handle (a psk_soft_handle_t *, owned by the component): psk_soft_peek, psk_soft_get_channel_stats ...
void *psk_harness_handle(void *hv)
{
    Harness *h = (Harness *)hv;
    return h->comp ? h->comp->handle() : h->comp_s ? h->comp_s->handle() : h->comp_c->handle();
}

}  // extern "C"
