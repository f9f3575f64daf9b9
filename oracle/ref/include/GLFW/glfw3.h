/*
 * GLFW/glfw3.h — stand-in for GLFW and the OpenGL 1.1 calls the reference
 * makes (TEST INFRASTRUCTURE ONLY; this project's own text, see
 * oracle/ref/README.md).
 *
 * A "window" is the set of keys the harness holds down and a close flag:
 * glfwGetKey answers from that set, which is all controls() asks of it.
 * Drawing, timing and window management do nothing; no arithmetic passes
 * through this header.  The key codes are GLFW's public ones.
 */
#ifndef ORC_REF_GLFW3_H
#define ORC_REF_GLFW3_H

/* ---- GLFW ---------------------------------------------------------------- */
#define GLFW_FALSE 0
#define GLFW_TRUE 1
#define GLFW_RELEASE 0
#define GLFW_PRESS 1
#define GLFW_RESIZABLE 0x00020003

#define GLFW_KEY_SPACE 32
#define GLFW_KEY_A 65
#define GLFW_KEY_D 68
#define GLFW_KEY_S 83
#define GLFW_KEY_W 87
#define GLFW_KEY_ESCAPE 256
#define GLFW_KEY_RIGHT 262
#define GLFW_KEY_LEFT 263
#define GLFW_KEY_DOWN 264
#define GLFW_KEY_UP 265
#define GLFW_KEY_LEFT_SHIFT 340

struct GLFWwindow {
    const int* pressed; /* the keys held down */
    int pressed_count;
    int should_close;
};
struct GLFWmonitor;

inline int glfwInit() { return GLFW_TRUE; }
inline void glfwTerminate() {}
inline void glfwWindowHint(int, int) {}
inline GLFWmonitor* glfwGetPrimaryMonitor() { return nullptr; }
inline GLFWwindow* glfwCreateWindow(int, int, const char*, GLFWmonitor*, GLFWwindow*) { return nullptr; }
inline void glfwMakeContextCurrent(GLFWwindow*) {}
inline int glfwWindowShouldClose(GLFWwindow* w) { return w ? w->should_close : GLFW_TRUE; }
inline void glfwSetWindowShouldClose(GLFWwindow* w, int value) { w->should_close = value; }
inline void glfwSwapBuffers(GLFWwindow*) {}
inline void glfwPollEvents() {}
inline double glfwGetTime() { return 0.0; }
inline int glfwGetKey(GLFWwindow* w, int key) {
    for (int i = 0; i < w->pressed_count; i++)
        if (w->pressed[i] == key) return GLFW_PRESS;
    return GLFW_RELEASE;
}

/* ---- OpenGL 1.1 ------------------------------------------------------------ */
typedef unsigned int GLenum;
typedef unsigned int GLuint;
typedef unsigned int GLbitfield;
typedef int GLint;
typedef int GLsizei;
typedef float GLfloat;
typedef unsigned char GLubyte;

#define GL_QUADS 0x0007
#define GL_TEXTURE_2D 0x0DE1
#define GL_UNSIGNED_BYTE 0x1401
#define GL_RGBA 0x1908
#define GL_VERSION 0x1F02
#define GL_NEAREST 0x2600
#define GL_TEXTURE_MAG_FILTER 0x2800
#define GL_TEXTURE_MIN_FILTER 0x2801
#define GL_COLOR_BUFFER_BIT 0x00004000

inline void glEnable(GLenum) {}
inline void glGenTextures(GLsizei n, GLuint* textures) {
    for (GLsizei i = 0; i < n; i++) textures[i] = (GLuint)(i + 1);
}
inline void glBindTexture(GLenum, GLuint) {}
inline void glTexParameteri(GLenum, GLenum, GLint) {}
inline void glTexImage2D(GLenum, GLint, GLint, GLsizei, GLsizei, GLint, GLenum, GLenum, const void*) {}
inline void glBegin(GLenum) {}
inline void glEnd() {}
inline void glTexCoord2f(GLfloat, GLfloat) {}
inline void glVertex2f(GLfloat, GLfloat) {}
inline void glFinish() {}
inline void glClear(GLbitfield) {}
inline const GLubyte* glGetString(GLenum) { return reinterpret_cast<const GLubyte*>("none (CPU stand-in)"); }

#endif
