// switches.hip — reads the A/B environment switches (switches.h) once, when the library is loaded, from ONE table, and
// describes what it read. No other unit calls getenv.
#include "common.h"
#include <cstdlib>

namespace yolo {

// (field of Switches, variable, rule, value when the variable is not set), in the order of INTEGRATION.md's table.
//   Set      true when the variable exists at all, whatever its value ("0" and "" included)
//   NotZero  false only when the value's first character is '0'
//   Int      atoi of the value        Long      atoll of the value
#define YOLO_SWITCH_TABLE(X)                                       \
    X(no_dma,            "YOLO_NO_DMA",            Set,     0)     \
    X(no_s2_dma,         "YOLO_NO_S2_DMA",         Set,     0)     \
    X(no_s2g,            "YOLO_NO_S2G",            Set,     0)     \
    X(no_stagger,        "YOLO_NO_STAGGER",        Set,     0)     \
    X(no_winograd,       "YOLO_NO_WINOGRAD",       Set,     0)     \
    X(no_conv3_ws,       "YOLO_NO_CONV3_WS",       Set,     0)     \
    X(no_conv1_rs,       "YOLO_NO_CONV1_RS",       Set,     0)     \
    X(no_wgrad_dma,      "YOLO_NO_WGRAD_DMA",      Set,     0)     \
    X(no_stem_wgrad,     "YOLO_NO_STEM_WGRAD",     Set,     0)     \
    X(stem_valu,         "YOLO_STEM_VALU",         Set,     0)     \
    X(f32_prio,          "YOLO_F32_PRIO",          NotZero, 1)     \
    X(dma_prio,          "YOLO_DMA_PRIO",          NotZero, 1)     \
    X(wgrad_la,          "YOLO_WGRAD_LA",          Int,     3)     \
    X(wgrad_prio,        "YOLO_WGRAD_PRIO",        Int,     0)     \
    X(stem_wgrad_blocks, "YOLO_STEM_WGRAD_BLOCKS", Int,     256)   \
    X(wino2_maxpix,      "YOLO_WINO2_MAXPIX",      Long,    256)

static bool read_Set(const char* v, bool unset) { return v ? true : unset; }
static bool read_NotZero(const char* v, bool unset) { return v ? v[0] != '0' : unset; }
static int read_Int(const char* v, int unset) { return v ? atoi(v) : unset; }
static long long read_Long(const char* v, long long unset) { return v ? atoll(v) : unset; }

static Switches read_switches() {
    Switches s;
#define X(field, name, rule, unset) s.field = read_##rule(getenv(name), unset);
    YOLO_SWITCH_TABLE(X)
#undef X
    return s;
}

const Switches g_switches = read_switches();

}  // namespace yolo

extern "C" int yolo_switches_describe(char* buf, size_t cap) {
    const yolo::Switches& s = yolo::switches();
    size_t n = 0;
#define X(field, name, rule, unset) \
    n += snprintf(buf && n < cap ? buf + n : nullptr, buf && n < cap ? cap - n : 0, "%s=%lld\n", name, (long long)s.field);
    YOLO_SWITCH_TABLE(X)
#undef X
    return (int)n;
}
