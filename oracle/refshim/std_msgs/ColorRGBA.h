// Stand-in message struct (TEST INFRASTRUCTURE ONLY; see ../ros/ros.h).
#ifndef F110_REFSHIM_COLORRGBA_H
#define F110_REFSHIM_COLORRGBA_H
namespace std_msgs {
struct ColorRGBA { float r = 0, g = 0, b = 0, a = 0; };
}
#endif
